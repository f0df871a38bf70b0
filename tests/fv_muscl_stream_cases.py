"""The case tables of the plane-streaming MUSCL-Hancock kernel (fv_muscl_stream_kernel, exahype_amd/csrc/exa_fv_muscl.hpp; a plan of
exa_fv_plan_create_streamed), shared by the CPU checks (tests/test_fv_muscl_stream_reference.py) and the GPU tests
(tests/test_fv_muscl_stream_kernels.py).  All rows are 3-D; a row is a row of tests/fv_muscl_cases.py: (dim, P, H, n_real, n_aux, n_patches,
pde, note), so that its states, its CFL step and its ids come from there.

The streamed plan (fv_muscl_stream_plan, exa_launch.hpp): a ring of window planes (P + 4)^2 V and three predictor planes (P + 2)^2 n_real, 8 B
each; five window planes are needed, a sixth is taken where it fits 160 KiB (it saves one of three barriers per plane), 256 threads.

EQUAL_SHAPES: where the resident kernel serves the shape too, the streamed one must give the same bits (the per-volume arithmetic is one set
of device functions).  What the shapes reach:

  P = 1, 2           the ring (6 slots) is deeper than the interior (T = 5, 6 window planes: no slot is ever reused at P = 1, one at P = 2)
  P = 3, 4, 5        slots are reused; window planes of 245 .. 405 doubles: odd and even lengths, i.e. both branches of the 16-byte staging
                     (a plane that starts 8 bytes off a 16-byte boundary in HBM or in LDS) and its scalar fallback
  P = 8, 5 + 1       the largest resident plan (122 944 B); 64 interior and 100 predictor tasks per plane
  P = 3, H = 3       the window planes are cut out of the patch row by row
  advection          n_real = 1 (+ 4 auxiliary), 5 of 8, and all 8 variables
each with 1 and with 5 patches, through the three entries.

STREAM_ROWS: shapes only the streamed plan serves.  P = 10 is the first one (resident: 178 880 B); P = 11 and 15 are the limiter's patches at
N = 6 and 8; P = 15 with an auxiliary variable; P = 19 is the largest plan at 5 + 0 variables and the one row that runs on FIVE window planes
(158 720 B; six would need 179 880 B), 361 interior and 441 predictor tasks per plane: two passes of the 256 threads; advection P = 12 with
all 8 variables; P = 11 at H = 3 (row staging).  Two or three patches each.
"""
from tests import fv_muscl_cases as K

E, A = K.E, K.A
LDS_AVAILABLE = 160 * 1024
ENTRIES = K.ENTRIES

# (P, H, n_real, n_aux, pde)
EQUAL_SHAPES = [
    (1, 2, 5, 0, E),
    (2, 2, 5, 0, E),
    (3, 2, 5, 0, E),
    (4, 2, 5, 0, E),
    (5, 2, 5, 0, E),
    (8, 2, 5, 1, E),
    (3, 3, 5, 1, E),
    (4, 2, 1, 4, A),
    (5, 2, 5, 0, A),
    (3, 2, 8, 0, A),
]
EQUAL_COUNTS = (1, 5)

STREAM_ROWS = [
    (3, 10, 2, 5, 0, 2, E, "the first shape without a resident plan"),
    (3, 11, 2, 5, 0, 3, E, "the limiter's patch at N = 6"),
    (3, 15, 2, 5, 0, 2, E, "the limiter's patch at N = 8"),
    (3, 15, 2, 5, 1, 2, E, ""),
    (3, 19, 2, 5, 0, 2, E, "five window planes; two passes of the threads per plane"),
    (3, 12, 2, 8, 0, 2, A, ""),
    (3, 11, 3, 5, 0, 3, E, "H > 2"),
]


def equal_row(shape, n):
    P, H, n_real, n_aux, pde = shape
    return (3, P, H, n_real, n_aux, n, pde, "")


def shape_id(shape):
    return K.row_id(equal_row(shape, 0)).replace("-n0", "")


def stream_need(P, n_real, V):
    """bytes of five window planes and three predictor planes: what a streamed plan needs at least"""
    return 8 * (5 * (P + 4) ** 2 * V + 3 * (P + 2) ** 2 * n_real)


def stream_plan(P, n_real, V):
    """fv_muscl_stream_plan (exa_launch.hpp) restated: (ring depth, threads, LDS bytes); None where five + three planes exceed 160 KiB"""
    five = stream_need(P, n_real, V)
    if five > LDS_AVAILABLE:
        return None
    six = five + 8 * (P + 4) ** 2 * V
    return (6, 256, six) if six <= LDS_AVAILABLE else (5, 256, five)
