"""Lane tables for the register-resident stage A (exa_dg_reg.hpp): development aid, not part of the product.

The derive phase of that kernel gives every lane one pencil task (direction d, level slot ls, pencil t) of a two-level step, directions
mixed inside a wave.  A wave instruction "node jj of my pencil" is bank-conflict-free iff, inside each hardware lane group, the addresses
base(d, ls, t) + jj * stride(d) fall on distinct banks (MI355X_MICROARCH.md LDS table: ds_read_b64 = 2 groups of 32 lanes over 32
double-banks; ds_write_b64 = 4 groups of 16 contiguous lanes over 16 double-banks, free while the array cycles stay <= 6).
This script searches the strides (PY, PX, SL) that fit two workgroups into the 160 KiB and, by annealing, the lane -> task assignment;
it reports the extra LDS cycles per step and prints the tables as C initialisers.  The C++ side (dg_inst.hip fill_reg_tables) holds a
deterministic constructive version of the same model; this script is what showed which layout it has to aim at.

The primitive image (exa_dg_reg.hpp StageAReg::PUT: the owners put NPUT = 6 values per node, a pencil task reads them and, a second time, the
normal component from slot PUT_VN + d of ITS direction) adds one read per node whose slot differs between the lanes of a group that mixes
directions: `library_table` restates the constructive tables of dg_inst.hip fill_reg_tables (8-byte layout), `step_cost` prices a two-level
step of a table under either image, the second read included.

usage: reg_tables.py [N] [iters]        the search
       reg_tables.py model              modelled conflict cycles per step of the shipped table, both images, and of the closing phases'
                                        volume rounds for the array strides 216 and 217 of the closing image (volume_cost)
"""
import random
import sys

ARGS = sys.argv[1:] if __name__ == "__main__" else []        # (imported -- tests/test_reg_tables_model.py: the defaults)
N = int(ARGS[0]) if len(ARGS) > 0 and ARGS[0].isdigit() else 6
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 200000
NV, NA, LG = 5, 2, 2
NF, NN = N * N, N * N * N
LDS_DOUBLES = (160 * 1024 // 2 - 512) // 8         # per workgroup, two per CU, a little slack for static arrays


def geometry(PY, PX, SL):
    ps = (PX, PY, 1)

    def pbase(d, t):
        a, b = divmod(t, N)
        return (a * PY + b, a * PX + b, a * PX + b * PY)[d]

    def node_off(n):
        return (n // NF) * PX + ((n // N) % N) * PY + n % N
    return ps, pbase, node_off


def group_cost(addrs, lanes, banks):
    """LDS array cycles of one wave instruction: per lane group the largest number of distinct addresses on one bank."""
    cyc = 0
    for g in range(0, 64, lanes):
        per = {}
        for a in addrs[g:g + lanes]:
            if a is not None:
                per.setdefault(a % banks, set()).add(a)
        cyc += max((len(v) for v in per.values()), default=0) if per else 0
    return cyc


def derive_cost(assign, PY, PX, SL, detail=False):
    """extra LDS cycles of the derive phase of one two-level step: reads (7 per node: 5 variables + 2 cached scalars) and writes (5 per node)"""
    ps, pbase, _ = geometry(PY, PX, SL)
    QSZ = NV * LG * SL
    rd = wr = 0
    for w in range(4):
        lanes = assign[64 * w:64 * w + 64]
        for jj in range(N):
            ra = [None if t is None else t[1] * SL + pbase(t[0], t[2]) + jj * ps[t[0]] for t in lanes]
            wa = [None if t is None else t[1] * SL + pbase(t[0], t[2]) + jj * ps[t[0]] + t[0] * QSZ for t in lanes]
            rd += (NV + NA) * max(0, group_cost(ra, 32, 32) - 2)
            wr += NV * max(0, group_cost(wa, 16, 16) - 6)
    return (rd, wr) if detail else rd + wr


NPUT, PUT_VN = 6, 0                                # exa_pde.hpp Euler: m_x, m_y, m_z, 1/rho, E + p, p; normal momentum of direction d in slot PUT_VN + d


def library_geometry():
    """strides of exa_dg_reg.hpp RegGeo<N>: unpadded rows and planes, odd level stride"""
    return N, N * N, NN + (1 if NN % 2 == 0 else 0)


def library_table(nl=2):
    """lane -> (d, ls, t) or None: dg_inst.hip fill_reg_tables restated (8-byte layout), nl levels in the step"""
    PY, PX, SL = library_geometry()
    _, pbase, _ = geometry(PY, PX, SL)
    ps = (PX, PY, 1)
    QSZ, NT, NG = NV * LG * SL, 256, 8

    def base(k):
        return k[1] * SL + pbase(k[0], k[2])
    out = [None] * NT
    groups = []
    for d in range(3):
        byres = [[] for _ in range(32)]
        for ls in range(nl):
            for t in range(NF):
                byres[base((d, ls, t)) & 31].append((d, ls, t))
        g = 0
        while True:
            grp = [b[g] for b in byres if len(b) > g]
            if not grp:
                break
            groups.append(grp)
            g += 1
    groups.sort(key=lambda grp: -len(grp))             # (stable, as std::stable_sort)
    npure = min(len(groups), NG)
    while npure > 0 and sum(len(g) for g in groups[npure:]) > 32 * (NG - npure):
        npure -= 1
    for g in range(npure):
        for k in groups[g]:
            out[32 * g + (base(k) & 31)] = k

    def group_score(g):
        score = 0
        for jj in range(N):
            seen_r, seen_w = {}, {}
            for lane in range(32):
                k = out[32 * g + lane]
                if k is None:
                    continue
                a = base(k) + jj * ps[k[0]]
                w = a + k[0] * QSZ
                seen_r.setdefault(a & 31, set()).add(a)
                seen_w.setdefault((lane // 16, w & 15), set()).add(w)
            mr = max([1] + [len(v) for v in seen_r.values()])
            mw = [max([1] + [len(v) for (h, _), v in seen_w.items() if h == half]) for half in range(2)]
            score += 2 * (NV + NA) * (mr - 1) + NV * (mw[0] - 1 + mw[1] - 1)
        return score
    for grp in groups[npure:]:
        for k in grp:
            best_lane, best = -1, 1 << 30
            for lane in range(32 * npure, NT):
                if out[lane] is not None:
                    continue
                before = group_score(lane // 32)
                out[lane] = k
                delta = group_score(lane // 32) - before
                out[lane] = None
                if delta < best:
                    best, best_lane = delta, lane
            out[best_lane] = k
    return out


def step_cost(assign, put):
    """Modelled extra LDS cycles of the derive phase of one two-level step of the library's geometry (the measure of derive_cost), as a dict:
    `same` = the reads every lane makes at the same slot (7 per node for the image q | 1/rho | p, NPUT for the primitive image), `vn` = the second
    read of the normal component (primitive image only: slot PUT_VN + d, i.e. a bank shift of (PUT_VN + d) * LG * SL doubles per direction),
    `wr` = the stores of the sums (their arrays lie QSZ apart whatever the image: a common shift changes no conflict)."""
    PY, PX, SL = library_geometry()
    ps, pbase, _ = geometry(PY, PX, SL)
    VS, QSZ = LG * SL, NV * LG * SL
    same = vn = wr = 0
    for w in range(4):
        lanes = assign[64 * w:64 * w + 64]
        for jj in range(N):
            ra = [None if t is None else t[1] * SL + pbase(t[0], t[2]) + jj * ps[t[0]] for t in lanes]
            va = [None if t is None else a + (PUT_VN + t[0]) * VS for t, a in zip(lanes, ra)]
            wa = [None if t is None else a + t[0] * QSZ for t, a in zip(lanes, ra)]
            same += (NPUT if put else NV + NA) * max(0, group_cost(ra, 32, 32) - 2)
            if put:
                vn += max(0, group_cost(va, 32, 32) - 2)
            wr += NV * max(0, group_cost(wa, 16, 16) - 6)
    return dict(same=same, vn=vn, wr=wr, total=same + vn + wr)


def volume_cost(FS):
    """Modelled extra LDS cycles of the closing phases' volume rounds of one cell (exa_dg_reg.hpp: one round per direction, lane = task (v, t), t
    fastest, NV * NF of the 256 lanes at work) for a closing image [array][variable][node] of array stride FS, as a dict: `rd` = the loads of qbar
    and Fbar_d (12 per lane and round; the two arrays lie a common shift apart, which changes no conflict), `wr` = the stores of the volume terms (6).
    Same measure as step_cost: cycles beyond the 2 (reads) or 6 (writes) a wave instruction takes without a conflict."""
    PY, PX, _ = library_geometry()
    ps, pbase, _ = geometry(PY, PX, 0)
    rd = wr = 0
    for w in range(4):
        lanes = [tid if tid < NV * NF else None for tid in range(64 * w, 64 * w + 64)]
        for d in range(3):
            for jj in range(N):
                a = [None if tid is None else (tid // NF) * FS + pbase(d, tid % NF) + jj * ps[d] for tid in lanes]
                rd += 2 * max(0, group_cost(a, 32, 32) - 2)
                wr += max(0, group_cost(a, 16, 16) - 6)
    return dict(rd=rd, wr=wr, total=rd + wr)


def mixed_groups(assign):
    """the 32-lane groups of a table that hold pencils of more than one direction"""
    return [g for g in range(len(assign) // 32) if len({t[0] for t in assign[32 * g:32 * g + 32] if t is not None}) > 1]


def owner_cost(order, PY, PX, SL):
    _, _, node_off = geometry(PY, PX, SL)
    rd = wr = 0
    for w in range(4):
        a = [None if n is None else node_off(n) for n in order[64 * w:64 * w + 64]]
        rd += max(0, group_cost(a, 32, 32) - 2)
        wr += max(0, group_cost(a, 16, 16) - 6)
    return rd, wr


def anneal(PY, PX, SL, iters, seed=1):
    rng = random.Random(seed)
    tasks = [(d, ls, t) for d in range(3) for ls in range(LG) for t in range(NF)]
    assign = tasks + [None] * (256 - len(tasks))
    rng.shuffle(assign)
    cur = derive_cost(assign, PY, PX, SL)
    best, best_assign = cur, list(assign)
    T = 8.0
    for it in range(iters):
        i, j = rng.randrange(256), rng.randrange(256)
        if assign[i] is None and assign[j] is None:
            continue
        assign[i], assign[j] = assign[j], assign[i]
        c = derive_cost(assign, PY, PX, SL)
        if c <= cur or rng.random() < pow(2.718281828, -(c - cur) / T):
            cur = c
            if c < best:
                best, best_assign = c, list(assign)
                if best == 0:
                    break
        else:
            assign[i], assign[j] = assign[j], assign[i]
        T = max(0.05, T * 0.99997)
    return best, best_assign


def owner_order(PY, PX, SL):
    """owner slot -> node: greedy, 32-lane groups with distinct residues mod 32 whose 16-lane halves are distinct mod 16"""
    _, _, node_off = geometry(PY, PX, SL)
    left = list(range(NN))
    order = []
    while left:
        grp, used32 = [], set()
        for half in range(2):
            used16 = set()
            for n in list(left):
                r = node_off(n)
                if r % 32 not in used32 and r % 16 not in used16 and len(used16) < 16:
                    used32.add(r % 32)
                    used16.add(r % 16)
                    grp.append(n)
                    left.remove(n)
            grp += [None] * (16 * (half + 1) - len(grp))
        order += grp
    order += [None] * (256 - len(order))
    return order[:256] if len(order) >= 256 else order


if __name__ == "__main__" and ARGS[:1] == ["model"]:
    tab = library_table(2)
    old, new = step_cost(tab, False), step_cost(tab, True)
    print("shipped table, two-level step: groups that mix directions %s" % mixed_groups(tab))
    print("image q | 1/rho | p : modelled extra LDS cycles per step %s" % old)
    print("primitive image     : modelled extra LDS cycles per step %s" % new)
    for FS in (NN, library_geometry()[2]):
        print("volume rounds, closing image of array stride %d: modelled extra LDS cycles per cell %s" % (FS, volume_cost(FS)))
    sys.exit(0)
if __name__ == "__main__":
    cands = []
    for PY in (N, N + 1):
        for PX in range(N * PY, N * PY + 5):
            for SL in range(N * PX, N * PX + 9):
                if (NV + NA + 3 * NV) * LG * SL <= LDS_DOUBLES:
                    cands.append((PY, PX, SL))
    print("candidates that fit two workgroups per CU:", cands)
    quick = []
    for (PY, PX, SL) in cands:
        c, a = anneal(PY, PX, SL, ITERS // 20)
        order = owner_order(PY, PX, SL)
        oc = owner_cost(order, PY, PX, SL) if len(order) == 256 else (99, 99)
        quick.append((c + 30 * sum(oc), c, oc, PY, PX, SL))
        print("PY %d PX %d SL %d: derive extra cycles/step %d, owner extra (rd, wr) %s" % (PY, PX, SL, c, oc), flush=True)
    quick.sort()
    _, _, _, PY, PX, SL = quick[0]
    best, assign = anneal(PY, PX, SL, ITERS, seed=7)
    order = owner_order(PY, PX, SL)
    print("best: PY %d PX %d SL %d, derive extra cycles per step (rd, wr) %s, owner %s" %
          (PY, PX, SL, derive_cost(assign, PY, PX, SL, True), owner_cost(order, PY, PX, SL)))
    print("// lane -> derive task (d | ls << 2 | t << 3), -1 idle")
    print(", ".join(str(-1 if t is None else t[0] | t[1] << 2 | t[2] << 3) for t in assign))
    print("// owner slot -> node, -1 idle")
    print(", ".join(str(-1 if n is None else n) for n in order))
