"""The SPD inverse on matrices whose inverse is known exactly (tests/inverse_model.py): every path must return X_s bit for bit, and the
index of a non-positive pivot that the SWEEP reports (CHOLESKY=0: no fallback answers in its place) must be LAPACK's, k + 1, wherever
the pivot sits -- every block of every group, the ramp, the ragged last block, row n itself.

Every assertion is integer equality or array_equal; the one bound (log det) is derived where it is used."""
import math
import time

import numpy as np
import pytest

import inverse_model as im
from gdca_testutil import _SCHEDULES, g  # noqa: F401 (fixture)
from oracle import gdca_oracle as o

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KINDS = ("neg", "zero")
N_RAMP = 1752   # 14 blocks, 88 real rows in the last: the smallest block count at which the ramp of groups of four engages


def _ids(opts):
    return ",".join("%s=%s" % (k[5:] if k.startswith("GDCA_") else k, v) for k, v in opts.items()) or "default"


def context(g, opts, **more):
    c = g.Context(0)
    c.set_options(**opts)
    c.set_options(**more)
    return c


_dev = {}


def on_device(n):
    """(A_s, X_s) of im.family(n) as n x n device tensors (symmetric: either memory order), uploaded once"""
    import torch

    if n not in _dev:
        A, X, _ = im.family(n)
        _dev[n] = (torch.from_numpy(A).cuda(), torch.from_numpy(X).cuda())
        torch.cuda.synchronize()
    return _dev[n]


def inverse_in_place(c, M):
    """gdca_spd_inverse_dev on the device tensor M (raises PosDefException); the tensor's producer has finished first"""
    import torch

    from gaussdca.jl_amd import devops

    torch.cuda.synchronize()
    devops.inv_cholesky_dev(c, M.data_ptr(), M.shape[0])
    return M


def with_bad_pivot(n, k, kind, B=None):
    """im.bad_pivot of im.family(n) on the device: a clone of A_s (or the tensor B, in place) with the diagonal entry of row k replaced"""
    A, _, e = im.family(n)
    B = on_device(n)[0].clone() if B is None else B
    B[k, k] = im.bad_diagonal(A[k, k], e[k], kind)
    return B


def sizes_under(opts, n, merged=False):
    """the pivot groups the plan takes for an n x n matrix under `opts` (labels of the positions: they change no assertion)"""
    nblk = (n + 127) // 128
    merged = merged or bool(int(opts.get("GDCA_SWEEP_DEBUG", 0)) & 8)
    if merged:
        grp = 4 if nblk >= 24 else (2 if nblk >= 12 else 1)
    else:
        grp = int(opts.get("GDCA_GROUP", im.auto_group(nblk)))
    return im.group_sizes(nblk, grp, ramp=opts.get("GDCA_RAMP", "1") != "0")


# ---- A. the bits, every schedule ----------------------------------------------------------------------------------------------------
def logdet_close(n, e, value):
    """log det A_s = sum_k log 4^e_k = 2 ln 2 sum e_k.  The device sums n logarithms of exact powers of two (k_logdet): the bound of an
    n-term sum of correctly rounded terms, n u |logdet| + n u."""
    want = 2.0 * math.log(2.0) * float(np.sum(e))
    bound = n * U * abs(want) + n * U
    print("n=%d: logdet %+.17e, 2 ln2 sum e %+.17e, |difference| / bound = %.3g" % (n, value, want, abs(value - want) / bound))
    return abs(value - want) <= bound


@pytest.mark.parametrize("opts", _SCHEDULES, ids=_ids)
def test_every_schedule_returns_the_exact_inverse(g, opts):
    """n = 129, 300, 1100 and 1752 under every schedule, and at 1752 the three rungs of the recovery ladder: no step (REFINE=0), the
    Newton-Schulz step forced (REFINE=1: X + X (I - A X) = X + X 0), the Cholesky fallback forced (CHOLESKY=2: potrf + potri, exact on
    this input) -- the same bits."""
    c = context(g, opts)
    try:
        for n in (129, 300, 1100, N_RAMP):
            A, X, e = im.family(n)
            got = g.inv_cholesky(A, ctx=c)
            assert np.array_equal(got, X), (opts, n, int(np.count_nonzero(got != X)))
        n = N_RAMP
        A, X, e = im.family(n)
        got, ld = g.inv_cholesky(A, ctx=c, return_logdet=True)
        assert np.array_equal(got, X) and logdet_close(n, e, ld) and c.last_logdet(return_source=True) == (ld, 0)
        for switch in (dict(REFINE=0), dict(REFINE=1), dict(REFINE=-1, CHOLESKY=2)):
            c.set_options(**switch)
            got, ld = g.inv_cholesky(A, ctx=c, return_logdet=True)
            assert np.array_equal(got, X), (opts, switch, int(np.count_nonzero(got != X)))
            assert logdet_close(n, e, ld), (opts, switch)
            assert c.last_logdet(return_source=True) == (ld, 1 if "CHOLESKY" in switch else 0), (opts, switch)
    finally:
        c.close()


# ---- B. the sweep's own info ------------------------------------------------------------------------------------------------------
SWEEP_INFO = [(N_RAMP, {"GDCA_GROUP": "1"}), (N_RAMP, {"GDCA_GROUP": "2"}), (N_RAMP, {"GDCA_GROUP": "3"}), (N_RAMP, {"GDCA_GROUP": "4"}),
              (N_RAMP, {"GDCA_GROUP": "4", "GDCA_RAMP": "0"}), (N_RAMP, {}), (N_RAMP, {"GDCA_SWEEP_DEBUG": "24"}), (N_RAMP, {"GDCA_SLAB": "0"}),
              (300, {}), (300, {"GDCA_SWEEP_DEBUG": "24"})]


_oracle = {}


def oracle_infos(n, kind):
    """{k: LAPACK's info for im.family(n) with a bad pivot of `kind` at row k}, every row of im.positions(n); asked once per run of the
    suite (dpotrf stops at the bad pivot)"""
    if (n, kind) not in _oracle:
        A, _, e = im.family(n)
        B = A.copy()
        table = {}
        for k, *_ in im.positions(n):
            B[k, k] = im.bad_diagonal(A[k, k], e[k], kind)
            with pytest.raises(o.NotPositiveDefinite) as ei:
                o.spd_inverse(B)
            table[k] = ei.value.info
            B[k, k] = A[k, k]
        assert np.array_equal(B, A)
        _oracle[(n, kind)] = table
    return _oracle[(n, kind)]


def expect_info(g, c, M, want, what):
    """the inverse of M fails with `want`, and the context's log det is NaN afterwards"""
    with pytest.raises(g.PosDefException) as ei:
        inverse_in_place(c, M)
    assert ei.value.info == want, (what, ei.value.info, want)
    assert math.isnan(c.last_logdet()), what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,opts", SWEEP_INFO, ids=lambda v: _ids(v) if isinstance(v, dict) else "n%d" % v)
def test_the_sweep_reports_the_first_bad_pivot(g, n, opts, kind):
    """CHOLESKY=0: the number raised is the one ChainStep::run and sweep_pivot wrote.  A bad pivot at the first, an interior and the last
    row of every 128-block and at row n - 1 (im.positions: every slot of every group, the ramp's groups and the ragged block among
    them) is reported as k + 1 = LAPACK's info for the same matrix (oracle_infos); of two bad rows in different groups the smaller is
    reported; after each failure the same context inverts the intact matrix to X_s and its log det was NaN in between."""
    import torch

    A_d, X_d = on_device(n)
    sizes = sizes_under(opts, n)
    pos = im.positions(n, sizes)
    lapack = oracle_infos(n, kind)
    c = context(g, opts, CHOLESKY=0)
    t0 = time.perf_counter()
    try:
        for k, blk, grp, slot in pos:
            what = (opts, n, kind, "row %d: block %d = slot %d of group %d (sizes %s)" % (k, blk, slot, grp, sizes))
            assert lapack[k] == k + 1, what
            expect_info(g, c, with_bad_pivot(n, k, kind), lapack[k], what)
            assert torch.equal(inverse_in_place(c, A_d.clone()), X_d), what
            assert not math.isnan(c.last_logdet())
        # two bad rows in different groups: the smaller one
        first_of = {}
        for k, blk, grp, slot in pos:
            first_of.setdefault(grp, []).append(k)
        groups = sorted(first_of)
        other = "zero" if kind == "neg" else "neg"
        for ga, gb in ((groups[0], groups[-1]), (groups[len(groups) // 2], groups[-1]), (groups[-2], groups[-1])) if len(groups) > 1 else ():
            k1, k2 = first_of[ga][1], first_of[gb][-1]
            B = with_bad_pivot(n, k1, kind, with_bad_pivot(n, k2, other))
            expect_info(g, c, B, k1 + 1, (opts, n, kind, "rows %d and %d" % (k1, k2)))
        assert torch.equal(inverse_in_place(c, A_d.clone()), X_d)
    finally:
        c.close()
    print("n=%d %s %s: %d positions, %.2f s" % (n, _ids(opts), kind, len(pos), time.perf_counter() - t0))


@pytest.mark.parametrize("kind", KINDS)
def test_the_fallback_reports_what_the_sweep_reports(g, kind):
    """The same positions with the default CHOLESKY=1 (the blocked potrf answers) beside CHOLESKY=0 (the sweep answers): one number"""
    n = N_RAMP
    c0, c1 = context(g, {}, CHOLESKY=0), context(g, {})
    try:
        for k, *_ in im.positions(n, sizes_under({}, n)):
            infos = []
            for c in (c0, c1):
                with pytest.raises(g.PosDefException) as ei:
                    inverse_in_place(c, with_bad_pivot(n, k, kind))
                infos.append(ei.value.info)
                assert math.isnan(c.last_logdet())
            assert infos == [k + 1, k + 1], (kind, k, infos)
    finally:
        c0.close()
        c1.close()


# ---- C. batch members -----------------------------------------------------------------------------------------------------------------
def test_a_batch_reports_the_failing_members_info_and_leaves_the_others_exact(g):
    """gdca_spd_inverse_batch_dev, three members (300, 1752, 129) on contexts with CHOLESKY=0 sharing one merged launch: a bad pivot in
    member 1's last group, then in member 2 (n = 129: its full block, then the single real row of its ragged one) -- the info raised
    is that member's, the other members' buffers are X_s."""
    import torch

    ns = (300, N_RAMP, 129)
    cs = [context(g, {}, CHOLESKY=0) for _ in ns]
    try:
        for member, k, kind in ((1, 1700, "neg"), (1, 1751, "zero"), (1, 1536, "zero"), (2, 77, "zero"), (2, 128, "neg"), (0, 299, "neg")):
            bufs = [on_device(n)[0].clone() for n in ns]
            with_bad_pivot(ns[member], k, kind, bufs[member])
            torch.cuda.synchronize()
            with pytest.raises(g.PosDefException) as ei:
                g.spd_inverse_batch_dev(cs, [b.data_ptr() for b in bufs], list(ns))
            assert ei.value.info == k + 1, (member, k, kind, ei.value.info)
            for m, n in enumerate(ns):
                if m != member:
                    assert torch.equal(bufs[m], on_device(n)[1]), (member, k, kind, m)
                    assert not math.isnan(cs[m].last_logdet())
            assert math.isnan(cs[member].last_logdet())
        bufs = [on_device(n)[0].clone() for n in ns]
        torch.cuda.synchronize()
        assert g.spd_inverse_batch_dev(cs, [b.data_ptr() for b in bufs], list(ns)) == [0, 0, 0]
        for m, n in enumerate(ns):
            assert torch.equal(bufs[m], on_device(n)[1]), m
    finally:
        for c in cs:
            c.close()


# ---- D. ragged tails --------------------------------------------------------------------------------------------------------------------
RAGGED_SIZES = tuple(256 + r for r in (1, 15, 16, 17, 111, 112, 113, 127)) + (16, 17, 127, 128)


@pytest.mark.parametrize("opts", [{}, {"GDCA_RAGGED": "0"}], ids=_ids)
def test_ragged_tails_are_exact_and_the_last_row_is_reported(g, opts):
    """The sweep skips the padding of the last block in units of 16 rows (plan_sweep: rl): remainders of 1, 15, 16, 17, 111, 112, 113
    and 127 rows behind two full blocks, and n = 16, 17, 127, 128 alone -- X_s bit for bit, and a bad LAST row (the idx <= n_real
    clause of sweep_pivot) reported as n."""
    c, c0 = context(g, opts), context(g, opts, CHOLESKY=0)
    try:
        for n in RAGGED_SIZES:
            A, X, e = im.family(n)
            for cc in (c, c0):
                got = g.inv_cholesky(A, ctx=cc)
                assert np.array_equal(got, X), (opts, n, int(np.count_nonzero(got != X)))
            for kind in KINDS:
                with pytest.raises(g.PosDefException) as ei:
                    g.inv_cholesky(im.bad_pivot(A, e, n - 1, kind), ctx=c0)
                assert ei.value.info == n, (opts, n, kind, ei.value.info)
                assert math.isnan(c0.last_logdet())
            assert np.array_equal(g.inv_cholesky(A, ctx=c0), X), (opts, n)
    finally:
        c.close()
        c0.close()


# ---- E. the automatic group rule at its switches --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5632, 5633, 6700, 7700], ids=lambda n: "n%d" % n)
def test_the_automatic_group_rule_is_exact_at_its_switches(g, n):
    """Default options: 44 blocks (the last size swept in single blocks), 45 (groups of two; one real row in the last block), 53
    (groups of three) and 61 (groups of four), each with the ramp and the remainder's insertion.  Built and compared on the device."""
    import torch

    nblk = (n + 127) // 128
    assert (nblk, im.auto_group(nblk)) in ((44, 1), (45, 2), (53, 3), (61, 4)) and im.auto_group(nblk - 1) == max(im.auto_group(nblk) - 1, 1)
    t0 = time.perf_counter()
    A, X, _ = im.exact_family_dev(n, 7000 + n)
    c = context(g, {})
    try:
        inverse_in_place(c, A)
        assert torch.equal(A, X), (n, int((A != X).sum()))
    finally:
        c.close()
    print("n=%d (%d blocks, groups %s ...): %.2f s" % (n, nblk, im.group_sizes(nblk, im.auto_group(nblk))[:6], time.perf_counter() - t0))


# ---- F. the fused path ------------------------------------------------------------------------------------------------------------------
def test_a_fused_run_raises_the_sweeps_info_and_the_fallbacks_alike(g):
    """An alignment with one constant column at pseudocount 0: the covariance rows of the symbols that column never shows are exactly
    zero, so the pivot of the first of them is exactly zero in any arithmetic -- row 160 (site 40 of q = 5: the second 128-block).
    gdca_run under CHOLESKY=0 (the sweep's number) and under the default (the fallback's) raise the oracle's info."""
    rng = np.random.default_rng(77)
    N, M, q = 60, 600, 5
    Zo = rng.integers(1, q + 1, size=(M, N)).astype(np.int8)     # every symbol and the gap at every site
    Zo[:, 40] = 2
    for a in range(1, q + 1):
        assert np.all(np.count_nonzero(np.delete(Zo, 40, axis=1) == a, axis=0) > 0)
    Pi_true, Pij_true, _, _ = o.compute_weighted_frequencies(np.ascontiguousarray(Zo), q, "auto")
    Pi, Pij = o.add_pseudocount(Pi_true, Pij_true, 0.0, q)
    with pytest.raises(o.NotPositiveDefinite) as ei:
        o.spd_inverse(o.compute_C(Pi, Pij))
    want = ei.value.info
    assert want == 40 * (q - 1) + 1
    Zf = np.asfortranarray(Zo.T)
    for more in (dict(CHOLESKY=0), {}):
        c = context(g, {}, **more)
        try:
            with pytest.raises(g.PosDefException) as ei:
                c.run(Zf, q, 0.0, -1.0, 0)
            assert ei.value.info == want, (more, ei.value.info, want)
            S, st = c.run(Zf, q, 0.5, -1.0, 0)                     # the context still works
            assert st["info"] == 0 and np.isfinite(S).all()
        finally:
            c.close()
