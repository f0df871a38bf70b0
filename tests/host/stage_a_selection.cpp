// Which stage-A kernel the ADER-DG units pick, printed for every (N, n_picard, variant) of every launch table, and a hash of the lane
// tables their operator images carry.  Pure host functions of the library (exa_launch.hpp: DgLaunchTable): no plan, no device.
// tests/test_stage_a_selection.py builds this against the tree's library and compares the output with tests/golden/stage_a_selection.txt,
// which was written by the same program from the library before the selection was brought into one function.
//
//   stage_a_selection [label=path/to/libexahype_user.so ...]      (side libraries of generated term sets: their exa_user_dg_table_{2,3})
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "exa_launch.hpp"

using exa::DgLaunchTable;
using exa::DgOpsHost;

// bytes of the operator block in front of the lane tables (dg_inst.hip: StageA::PERM_OFF)
static size_t perm_off(int N) {
    switch (N) {
#define X(n) case n: return (sizeof(exa::DgOps<n>) + 15) / 16 * 16;
        X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
    }
    return 0;
}

static uint64_t fnv1a(const unsigned char* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

static int report(const char* label, int dim, const DgLaunchTable* t) {
    if (!t) { printf("%s dim=%d: not built\n", label, dim); return 0; }
    for (int N = 2; N <= 8; N++) {
        DgOpsHost h;
        memset(&h, 0, sizeof(h));
        if (exa::build_dg_operators(N, &h) != 0) { fprintf(stderr, "build_dg_operators(%d) failed\n", N); return 1; }
        for (int n_it : {0, 1, 3})
            for (int variant = 0; variant <= 2; variant++) {
                h.stage_a_variant = variant;
                printf("%s dim=%d N=%d n_it=%d variant=%d name=%s has_stage_ba=%d scratch_bytes=%zu ops_image=%zu\n", label, dim, N, n_it, variant,
                       t->stage_a_name(N, n_it, variant), t->has_stage_ba(N, n_it, variant), t->scratch_bytes(N), t->ops_image(N, &h, nullptr));
            }
        if (dim == 3 && (N == 6 || N == 8)) {              // the orders whose images carry the lane tables of the reg / m8 kernels
            const size_t bytes = t->ops_image(N, &h, nullptr), off = perm_off(N);
            std::vector<unsigned char> img(bytes, 0);
            if (t->ops_image(N, &h, img.data()) != bytes || off > bytes) { fprintf(stderr, "ops_image(%d) size mismatch\n", N); return 1; }
            printf("%s dim=%d N=%d lane_tables bytes=%zu fnv1a64=%016llx\n", label, dim, N, bytes - off, (unsigned long long)fnv1a(img.data() + off, bytes - off));
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    static const int built[5][2] = {{3, 1}, {2, 1}, {2, 0}, {3, 2}, {2, 2}};
    for (auto& b : built) {
        char label[32];
        snprintf(label, sizeof(label), "pde=%d", b[1]);
        if (report(label, b[0], exa::dg_launch_table(b[0], b[1]))) return 1;
    }
    for (int a = 1; a < argc; a++) {
        char* eq = strchr(argv[a], '=');
        if (!eq) { fprintf(stderr, "usage: %s [label=library ...]\n", argv[0]); return 2; }
        *eq = 0;
        void* lib = dlopen(eq + 1, RTLD_NOW | RTLD_LOCAL);
        if (!lib) { fprintf(stderr, "dlopen(%s): %s\n", eq + 1, dlerror()); return 1; }
        for (int dim = 2; dim <= 3; dim++) {
            char sym[32];
            snprintf(sym, sizeof(sym), "exa_user_dg_table_%d", dim);
            auto fn = reinterpret_cast<const void* (*)()>(dlsym(lib, sym));
            if (report(argv[a], dim, fn ? static_cast<const DgLaunchTable*>(fn()) : nullptr)) return 1;
        }
    }
    return 0;
}
