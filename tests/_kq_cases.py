"""The walk shapes of the matrix-core dense-gate kernels: the case table of tests/test_gpu_kq_forms.py and a plain-Python
model of how each launch of launch_kq_mfma (qcmrf_amd/csrc/qsv_layout.inc) hands its batches to waves, written from the
launch arithmetic there and from the loops of k_kq_mfma, k_kq_mfma3, k_kq_mfma3w and k_kq_lds (qsv_kernels.h).

A dense gate on k targets (K = max(k, 4) index bits: three targets are padded with a free qubit) of a shard of L local
qubits is nbatch = 2^(L - K - 4) batches of 16 amplitude groups.  At the sizes a test can hold, nbatch and the grids are
small powers of two, so every wave gets 1, 4 or 16 batches; the option kq_grid (at most that many workgroups) makes a few
waves walk many batches, uneven shares included, the way a 27..34-qubit shard makes them.  tests/test_kq_cases.py checks
on the host that the rows below reach every shape listed there, and that the model -- with three mistakes planted in it --
would notice a batch handled twice, never, or fetched from past the end.

A row is (L, k, variant, kq_grid, chunked, nontemporal, swizzle): engine options kq_variant, kq_grid, kq_chunked,
nontemporal and swizzle on a shard of L local qubits (kq3_tile is 0 in every row: k = 3 runs padded on the matrix cores).
"""
from collections import namedtuple

WAVES = 4                                            # QSV_TPB / 64: waves per workgroup of every kernel but k_kq_lds<5, ., 6>
N_CU = (256, 304, 64)                                # the model is checked for these device sizes
MISTAKES = ("tail_first_slot_only", "fetch_not_clamped", "peeled_round_counted_again")

Row = namedtuple("Row", "L k variant kq_grid chunked nontemporal swizzle")
Launch = namedtuple("Launch", "kernel grid nw n pd prefetch fallback")
# one wave of a launch.  done: the batches (k_kq_mfma3w: steps) it computes and stores, in order; fetched: every index it
# loads; returned: it left at wave0 >= nbatch; n_my, peeled, rounds, tail: k_kq_lds -- its share, whether the peeled round
# ran, the loop bodies after it, the guarded steps; more: k_kq_mfma3 -- per batch, whether the next one was requested;
# chunk: (bt0, bt1, per) of the chunked walk
Wave = namedtuple("Wave", "wave0 returned done fetched n_my peeled rounds tail more chunk")


def km_of(k):
    return max(k, 4)


def nbatch_of(L, k):
    assert L - km_of(k) >= 4, "the matrix-core path needs 16 groups"
    return (1 << (L - km_of(k))) >> 4


def launch(L, k, variant, kq_grid, n_cu, blocks_per_cu=0):
    """the launch launch_kq_mfma<K> makes: kernel, workgroups, waves per workgroup, work items (batches; steps of two
    batches for k_kq_mfma3w), loads in flight (k_kq_lds), prefetch (k_kq_mfma3), and whether variant 5 fell back"""
    K, nb = km_of(k), nbatch_of(L, k)
    cap = (lambda g: min(g, kq_grid)) if kq_grid > 0 else (lambda g: g)
    if 6 <= variant <= 8:
        nw = 6 if (variant == 6 and K == 5) else 4
        bpc = blocks_per_cu if blocks_per_cu > 0 else (64 if K == 4 else 8)
        want = (nb + nw * 16 - 1) // (nw * 16)
        return Launch("lds", cap(max(1, min(want, n_cu * bpc))), nw, nb, variant - 5, False, False)
    bpc = blocks_per_cu if blocks_per_cu > 0 else 64
    if variant == 5 and nb % 2 == 0:
        nsteps = nb // 2
        return Launch("mfma3w", cap(max(1, min((nsteps + 15) // 16, n_cu * bpc))), WAVES, nsteps, 0, False, False)
    v = 3 if variant == 5 else variant
    grid = cap(max(1, min((nb + 31) // 32, n_cu * bpc)))
    return Launch("mfma" if v == 0 else "mfma3", grid, WAVES, nb, 0, v in (2, 3), variant == 5)


def walk_lds(la, wave0, mistake=None):
    """one wave of k_kq_lds<K, NT, NW, DBG, PD>: PD slots, fetches unconditional and clamped, the first round peeled"""
    n, pd, nwaves = la.n, la.pd, la.grid * la.nw
    if wave0 >= n:
        return Wave(wave0, True, [], [], 0, False, 0, 0, [], None)
    n_my = (n - wave0 + nwaves - 1) // nwaves
    slots, done, fetched = [None] * pd, [], []

    def fetch(p, kk):
        if mistake != "fetch_not_clamped":
            kk = min(kk, n_my - 1)
        slots[p] = wave0 + kk * nwaves
        fetched.append(slots[p])

    def step(p, kk, refill):
        done.append(slots[p])
        if refill:
            fetch(p, kk + pd)

    for p in range(pd):
        fetch(p, p)
    k0, peeled, rounds, tail = 0, False, 0, 0
    if n_my >= pd:
        peeled = True
        for p in range(pd):
            step(p, p, True)
        k0 = 0 if mistake == "peeled_round_counted_again" else pd
        while k0 + pd <= n_my:
            for p in range(pd):
                step(p, k0 + p, True)
            rounds += 1
            k0 += pd
    if pd > 1:
        for p in range(1 if mistake == "tail_first_slot_only" else pd):
            if k0 + p < n_my:
                step(p, k0 + p, False)
                tail += 1
    return Wave(wave0, False, done, fetched, n_my, peeled, rounds, tail, [], None)


def walk_mfma(la, wave0, chunked):
    """one wave of k_kq_mfma / k_kq_mfma3: grid-stride, or (kq_chunked) its own contiguous run of ``per`` batches; the
    batch in hand was loaded before its products start, the next one is requested (or, without PF, loaded afterwards)
    only when there is one (``more``)"""
    n, nwaves = la.n, la.grid * WAVES
    per = (n + nwaves - 1) // nwaves
    bt0 = wave0 * per if chunked else wave0
    bt1 = min(bt0 + per, n) if chunked else n
    bstep = 1 if chunked else nwaves
    done, fetched, more = [], [], []
    if bt0 < bt1 and la.kernel == "mfma3":
        fetched.append(bt0)
    bt = bt0
    while bt < bt1:
        if la.kernel == "mfma":
            fetched.append(bt)                       # k_kq_mfma loads inside the loop
        else:
            more.append(bt + bstep < bt1)
            if more[-1]:
                fetched.append(bt + bstep)
        done.append(bt)
        bt += bstep
    return Wave(wave0, False, done, fetched, len(done), False, 0, 0, more, (bt0, bt1, per) if chunked else None)


def walk_mfma3w(la, wave0):
    """one wave of k_kq_mfma3w: a grid-stride loop over steps of two batches"""
    nwaves = la.grid * WAVES
    done = list(range(wave0, la.n, nwaves))
    return Wave(wave0, False, done, list(done), len(done), False, 0, 0, [], None)


def waves_of(row, n_cu, mistake=None, blocks_per_cu=0):
    """(launch, its waves) of a row on a device of n_cu compute units"""
    la = launch(row.L, row.k, row.variant, row.kq_grid, n_cu, blocks_per_cu)
    out = []
    for w in range(la.grid * la.nw):
        if la.kernel == "lds":
            out.append(walk_lds(la, w, mistake))
        elif la.kernel == "mfma3w":
            out.append(walk_mfma3w(la, w))
        else:
            out.append(walk_mfma(la, w, row.chunked))
    return la, out


def defects(row, n_cu, mistake=None):
    """what is wrong with a row's walk: work items computed more or less than once, indices fetched that do not exist"""
    la, waves = waves_of(row, n_cu, mistake)
    count = [0] * la.n
    bad = []
    for w in waves:
        for b in w.done:
            if 0 <= b < la.n:
                count[b] += 1
            else:
                bad.append("wave %d computes %d of %d" % (w.wave0, b, la.n))
        bad += ["wave %d fetches %d of %d" % (w.wave0, b, la.n) for b in w.fetched if not 0 <= b < la.n]
    bad += ["item %d computed %d times" % (b, c) for b, c in enumerate(count) if c != 1]
    return bad


# ------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------
L_MAX = 17
ACCESS = ((0, 2), (1, 2), (0, 0))                    # (nontemporal, swizzle), dealt over the rows in turn


def uncapped_grid(L, k, variant):
    return launch(L, k, variant, 0, min(N_CU)).grid


def _rows():
    rows = []

    def add(L, k, variant, kq_grid, chunked):
        nt, swz = ACCESS[len(rows) % len(ACCESS)]
        rows.append(Row(L, k, variant, kq_grid, chunked, nt, swz))

    for k in (4, 5):
        for L in range(km_of(k) + 4, L_MAX + 1):
            for variant in range(9):
                # a cap is a row of its own only where it bites: 1 and 3 workgroups (4 and 12 waves: 12 divides no nbatch)
                grids = [0] + [g for g in (1, 3) if uncapped_grid(L, k, variant) > g]
                for g in grids:
                    add(L, k, variant, g, 0)
                    # the contiguous walk is an option of k_kq_mfma / k_kq_mfma3 (variants 0..4, and 5 where it falls back)
                    if variant <= 4 or (variant == 5 and nbatch_of(L, k) % 2):
                        add(L, k, variant, g, 1)
    # three targets are padded to K = 4: the kernels that K = 4 selects by itself, every size, the caps that bite
    for L in range(8, L_MAX + 1):
        for variant in (5, 6):
            for g in [0] + [g for g in (1, 3) if uncapped_grid(L, 3, variant) > g]:
                add(L, 3, variant, g, 0)
    return rows


ROWS = _rows()
# rows that failed on the GPU once, by name (none so far: every row of the table passed when it was first run)
REGRESSIONS = {}
