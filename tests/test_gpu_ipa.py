"""Iterative partner matching on the device (gdca_select_confident*, gdca_concat_pairs*, gdca_run_partner_ipa*, gDCA_partner_ipa)
through the C-ABI, against tests/ipa_model.py.

The two kernels between the rounds are held to the numpy model exactly (array_equal).  The loop is held to its CONTRACT: round r's
match and gap are bit for bit what gdca_run_partner_match returns for Z_r -- every Z_r rebuilt on the host from the traces with the
model's own select -- and its figures (rounds_out) to the traces.  Natives per round are compared with the record of
tests/golden/ipa_family.json, whose margins tests/test_ipa_cpu.py holds against the bars of ipa_model's docstring."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import ipa_model as im
import partner_model as pt
from gdca_testutil import ctx, g  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC, MAX_ROUNDS = 0.5, 12
F = {name: k for k, name in enumerate(im.IPA_FIELDS)}
GAPS = np.array([np.inf, 0.0, -0.0, 1.5, -2.0, 3.0, -np.inf, 0.25])   # a small set: ties are the rule


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the selection kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KA", [1, 63, 64, 65, 4096, 4097, 20000])
def test_selection_kernel_equals_the_model(ctx, KA):
    rng = np.random.default_rng(KA)
    gap = GAPS[rng.integers(0, len(GAPS), size=KA)]
    match = np.where(rng.random(KA) < 0.8, rng.integers(0, 1000, size=KA), -1).astype(np.int32)
    cand = int(np.sum(match >= 0))
    for n_take in sorted({0, 1, cand // 2, cand, cand + 7, -4}):
        sel, n = ctx.select_confident(match, gap, n_take)
        want, n_want = im.select(match, gap, n_take)
        assert n == n_want == min(max(n_take, 0), cand) and np.array_equal(sel, want), (KA, n_take)
    # everybody unmatched; everybody matched with one gap (the order is that of a)
    sel, n = ctx.select_confident(np.full(KA, -1, dtype=np.int32), gap, KA)
    assert n == 0 and np.all(sel == -1)
    sel, n = ctx.select_confident(np.zeros(KA, dtype=np.int32), np.zeros(KA), (KA + 1) // 2)
    assert n == (KA + 1) // 2 and np.array_equal(sel[:n], np.arange(n)) and np.all(sel[n:] == -1)
    # a NaN ranks first of all, as in compute_ranking
    if KA >= 63:
        gn = gap.copy()
        gn[KA // 2] = np.nan
        mn = np.abs(match)
        assert np.array_equal(ctx.select_confident(mn, gn, 1)[0], im.select(mn, gn, 1)[0]) and ctx.select_confident(mn, gn, 1)[0][0] == KA // 2


def test_selection_argument_checks(g, ctx):
    p, E = g._lib._p, g._lib.GDCA_EINVAL
    match, gap, sel, n = np.zeros(4, dtype=np.int32), np.zeros(4), np.full(4, 77, dtype=np.int32), C.c_int32(-5)
    lib = ctx.lib
    assert lib.gdca_select_confident(ctx.h, p(match), p(gap), 0, 1, p(sel), C.byref(n)) == E
    assert lib.gdca_select_confident(ctx.h, None, p(gap), 4, 1, p(sel), C.byref(n)) == E
    assert lib.gdca_select_confident(ctx.h, p(match), None, 4, 1, p(sel), C.byref(n)) == E
    assert lib.gdca_select_confident(ctx.h, p(match), p(gap), 4, 1, None, C.byref(n)) == E
    assert np.all(sel == 77) and n.value == -5
    assert lib.gdca_select_confident(ctx.h, p(match), p(gap), 4, 3, p(sel), None) == 0 and sel.tolist() == [0, 1, 2, -1]


# ---- the concat kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,split", [(2, 1), (7, 3), (60, 30), (61, 17)])
def test_concat_kernel_equals_the_model(g, ctx, N, split):
    rng = np.random.default_rng(N)
    KA, KB = 300, 211
    XA = np.asfortranarray(rng.integers(1, 22, size=(split, KA)).astype(np.int8))
    XB = np.asfortranarray(rng.integers(1, 22, size=(N - split, KB)).astype(np.int8))
    for n_sel in (1, 255, 256, 257):
        selA, selB = rng.integers(0, KA, size=n_sel).astype(np.int32), rng.integers(0, KB, size=n_sel).astype(np.int32)
        selA[0], selB[-1] = KA - 1, KB - 1
        want = im.concat(XA, XB, selA, selB)
        for col0 in (0, 3):
            M = col0 + n_sel + 2
            Z = np.full((N, M), 77, dtype=np.int8, order="F")
            ctx.concat_pairs(XA, XB, selA, selB, Z, col0)
            assert np.array_equal(Z[:, col0:col0 + n_sel], want), (n_sel, col0)
            assert np.all(Z[:, :col0] == 77) and np.all(Z[:, col0 + n_sel:] == 77)
            # the device form writes the columns in place
            dZ = g.DeviceBuffer.from_array(ctx, np.full((N, M), 77, dtype=np.int8, order="F"))
            bufs = [g.DeviceBuffer.from_array(ctx, a) for a in (XA, XB, selA, selB)]
            ctx.concat_pairs_dev(bufs[0].ptr, KA, bufs[1].ptr, KB, N, split, bufs[2].ptr, bufs[3].ptr, n_sel, dZ.ptr, col0)
            Zd = dZ.download((N, M), dtype=np.int8)
            assert np.array_equal(Zd, Z), (n_sel, col0)
            # an index out of range: GDCA_EINVAL, nothing outside the requested columns is touched (device form), nothing at all (host form)
            for side, bad in (("a", KA), ("a", -1), ("b", KB), ("b", -1)):
                sa, sb = selA.copy(), selB.copy()
                (sa if side == "a" else sb)[n_sel // 2] = bad
                Zb = np.full((N, M), 77, dtype=np.int8, order="F")
                with pytest.raises(g.ArgumentError):
                    ctx.concat_pairs(XA, XB, sa, sb, Zb, col0)
                assert np.all(Zb == 77)
            dsa = g.DeviceBuffer.from_array(ctx, sa)
            dsb = g.DeviceBuffer.from_array(ctx, sb)
            dZ.upload(np.full((N, M), 77, dtype=np.int8, order="F"))
            with pytest.raises(g.ArgumentError):
                ctx.concat_pairs_dev(bufs[0].ptr, KA, bufs[1].ptr, KB, N, split, dsa.ptr, dsb.ptr, n_sel, dZ.ptr, col0)
            Zd = dZ.download((N, M), dtype=np.int8)
            assert np.all(Zd[:, :col0] == 77) and np.all(Zd[:, col0 + n_sel:] == 77)
            for b in bufs + [dZ, dsa, dsb]:
                b.free()
    # argument checks: nothing runs
    p, lib, E = g._lib._p, ctx.lib, g._lib.GDCA_EINVAL
    Z = np.full((N, 4), 77, dtype=np.int8, order="F")
    s2 = np.zeros(2, dtype=np.int32)
    assert lib.gdca_concat_pairs(ctx.h, p(XA), KA, p(XB), KB, N, 0, p(s2), p(s2), 2, p(Z), 0) == E
    assert lib.gdca_concat_pairs(ctx.h, p(XA), KA, p(XB), KB, N, N, p(s2), p(s2), 2, p(Z), 0) == E
    assert lib.gdca_concat_pairs(ctx.h, p(XA), 0, p(XB), KB, N, split, p(s2), p(s2), 2, p(Z), 0) == E
    assert lib.gdca_concat_pairs(ctx.h, p(XA), KA, p(XB), KB, N, split, p(s2), p(s2), -1, p(Z), 0) == E
    assert lib.gdca_concat_pairs(ctx.h, p(XA), KA, p(XB), KB, N, split, p(s2), p(s2), 2, p(Z), -1) == E
    assert lib.gdca_concat_pairs(ctx.h, p(XA), KA, p(XB), KB, N, split, None, p(s2), 2, p(Z), 0) == E
    assert lib.gdca_concat_pairs(ctx.h, p(XA), KA, p(XB), KB, N, split, p(s2), p(s2), 2, None, 0) == E
    assert lib.gdca_concat_pairs(ctx.h, p(XA), KA, p(XB), KB, N, split, p(s2), p(s2), 0, p(Z), 1) == 0   # nothing to write
    assert np.all(Z == 77)


# ---- the loop through the C-ABI ------------------------------------------------------------------------------------------------------------
_pools = {}


def pools(q, N, split):
    if (q, N, split) not in _pools:
        _pools[(q, N, split)] = im.pools(q, N, split)
    return _pools[(q, N, split)]


def run_ipa(g, c, P, Zfix, seedA, seedB, n_inc=im.N_INC, max_rounds=MAX_ROUNDS, traces=True, pc=PC, **over):
    """gdca_run_partner_ipa as it is declared -> dict(rc, match, gap, mt, gt, rounds (max_rounds x fields), done, st)"""
    p = g._lib._p
    KA, KB = P["XA"].shape[1], P["XB"].shape[1]
    seedA, seedB = np.ascontiguousarray(seedA, dtype=np.int32), np.ascontiguousarray(seedB, dtype=np.int32)   # (alive until the call returns)
    a = dict(XA=p(P["XA"]), KA=KA, XB=p(P["XB"]), KB=KB, offA=p(P["offA"]), offB=p(P["offB"]), S=len(P["offA"]) - 1, N=P["N"], q=P["q"],
             split=P["split"], what=1, prm=C.byref(g._lib.Params(pc, -1.0, 0, 0)), Zfix=None if Zfix is None else p(Zfix),
             Mfix=0 if Zfix is None else Zfix.shape[1], seedA=p(seedA), seedB=p(seedB), n_seed=len(seedA), n_inc=n_inc,
             max_rounds=max_rounds)
    if "Zfix_ptr" in over:   # (the pointer alone, Mfix as it is)
        a["Zfix"] = over.pop("Zfix_ptr")
    a.update(over)
    rows = max(a["max_rounds"], 1)
    out = dict(match=np.full(KA, 77, dtype=np.int32), gap=np.full(KA, 7.5), mt=np.full((rows, KA), 77, dtype=np.int32),
               gt=np.full((rows, KA), 7.5), rounds=np.full((rows, len(F)), -9.0), st=g._lib.Stats())
    done = C.c_int32(-5)
    out["rc"] = c.lib.gdca_run_partner_ipa(c.h, a["XA"], a["KA"], a["XB"], a["KB"], a["offA"], a["offB"], a["S"], a["N"], a["q"], a["split"],
                                           a["what"], a["prm"], a["Zfix"], a["Mfix"], a["seedA"], a["seedB"], a["n_seed"], a["n_inc"],
                                           a["max_rounds"], over.get("match", p(out["match"])), p(out["gap"]), p(out["mt"]) if traces else None,
                                           p(out["gt"]) if traces else None, p(out["rounds"]), C.byref(done), C.byref(out["st"]))
    out["done"] = done.value
    return out


def partner_match(g, c, P, Z, pc=PC):
    """one gdca_run_partner_match on the training alignment Z -> (match, gap, packed E, logdet, stats)"""
    p = g._lib._p
    KA, KB = P["XA"].shape[1], P["XB"].shape[1]
    E = np.empty(pt.blocks_length(P["offA"], P["offB"]))
    match, gap, st = np.empty(KA, dtype=np.int32), np.empty(KA), g._lib.Stats()
    prm = g._lib.Params(pc, -1.0, 0, 0)
    Z = np.asfortranarray(Z, dtype=np.int8)
    c.check(c.lib.gdca_run_partner_match(c.h, p(Z), P["N"], Z.shape[1], P["q"], C.byref(prm), P["split"], p(P["XA"]), KA, p(P["XB"]), KB,
                                         p(P["offA"]), p(P["offB"]), len(P["offA"]) - 1, 1, p(E), p(match), p(gap), C.byref(st)))
    return match, gap, E, c.last_logdet(), st


def check_contract(g, c, P, Zfix, seedA, seedB, max_rounds=MAX_ROUNDS):
    """The loop on context c, then its host-driven reproduction on the same context: every Z_r from trace r - 1 with the model's select.
    Returns (the loop's result, the reproduction's packed E per round)."""
    res = run_ipa(g, c, P, Zfix, seedA, seedB, max_rounds=max_rounds)
    assert res["rc"] == 0, c.lib.gdca_last_error(c.h)
    done, mt, gt, R = res["done"], res["mt"], res["gt"], res["rounds"]
    assert 1 <= done <= max_rounds and c.last_logdet() == R[done - 1, F["logdet"]]
    Z = im.seed_alignment(Zfix, P["XA"], P["XB"], seedA, seedB)
    Es, KA = [], P["XA"].shape[1]
    blocks_of = lambda E: pt.unpack(E, P["offA"], P["offB"])  # noqa: E731
    spA = np.repeat(np.arange(len(P["offA"]) - 1), np.diff(P["offA"]))
    for r in range(1, done + 1):
        m, gp, E, logdet, st = partner_match(g, c, P, Z)
        assert np.array_equal(m, mt[r - 1]), r
        assert np.array_equal(bits(gp), bits(gt[r - 1])), r
        Es.append(E)
        Zn, sel, n = im.next_training_set(Zfix, P["XA"], P["XB"], mt[r - 1], gt[r - 1], r * im.N_INC)
        cand = int(np.sum(m >= 0))
        # rounds_out against the traces, exactly
        row = R[r - 1]
        assert row[F["M_train"]] == Z.shape[1] and row[F["candidates"]] == cand and row[F["n_sel"]] == n, (r, row)
        assert row[F["n_changed"]] == (cand if r == 1 else int(np.sum(mt[r - 1] != mt[r - 2]))), (r, row)
        assert bits(row[F["logdet"]]) == bits(logdet) and bits(row[F["Meff"]]) == bits(st.Meff) and bits(row[F["theta"]]) == bits(st.theta), r
        assert row[F["ms_fit"]] >= 0 and row[F["ms_match"]] >= 0 and row[F["ms_select"]] >= 0 and row[F["reserved"]] == 0
        # the total cost within the bound of any summation order of its terms: K_A u sum |E|
        blocks = blocks_of(E)
        terms = [float(blocks[spA[a]][a - P["offA"][spA[a]], m[a] - P["offB"][spA[a]]]) for a in np.nonzero(m >= 0)[0]]
        bound = KA * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
        err = abs(row[F["cost"]] - math.fsum(terms))
        print("round %2d: M %3d, selected %3d of %3d, changed %3d; |cost - fsum| / bound = %.3g" %
              (r, Z.shape[1], n, cand, row[F["n_changed"]], err / bound if bound else 0.0))
        assert err <= bound, (r, err, bound)
        Z = Zn
    # the stop rule, from the traces
    sel_n = [int(R[r, F["n_sel"]]) for r in range(done)]
    cands = [int(R[r, F["candidates"]]) for r in range(done)]
    stop = [r for r in range(2, done + 1) if sel_n[r - 2] == cands[r - 2]]
    assert done == max_rounds or stop == [done], (done, sel_n, cands)
    # the outputs are the last round's; rows past the last round are not written
    assert np.array_equal(res["match"], mt[done - 1]) and np.array_equal(bits(res["gap"]), bits(gt[done - 1]))
    assert np.all(mt[done:] == 77) and np.all(gt[done:] == 7.5) and np.all(R[done:] == -9.0)
    assert res["st"].M == int(R[done - 1, F["M_train"]]) and res["st"].refined == 0
    return res, Es


CASES = [(q, N, split, v) for q in (2, 5, 21) for N, split in ((7, 3), (60, 30)) for v in im.VARIANTS]


@pytest.mark.parametrize("q,N,split,var", CASES, ids=["q%d-N%d-s%d-%s" % c for c in CASES])
def test_the_contract_round_by_round(g, ctx, q, N, split, var):
    P = pools(q, N, split)
    assert P["XA"].shape[1] == 162 and P["XB"].shape[1] == 161 and len(P["seedA"]) == 5
    sizes = list(zip(np.diff(P["offA"]).tolist(), np.diff(P["offB"]).tolist()))
    assert (0, 3) in sizes and (2, 0) in sizes and (5, 3) in sizes
    Zfix, seedA, seedB = im.variant(P, var)
    res, _ = check_contract(g, ctx, P, Zfix, seedA, seedB)
    # max_rounds = 1 is one gdca_run_partner_match on the seed alignment
    one = run_ipa(g, ctx, P, Zfix, seedA, seedB, max_rounds=1)
    m, gp = partner_match(g, ctx, P, im.seed_alignment(Zfix, P["XA"], P["XB"], seedA, seedB))[:2]
    assert one["rc"] == 0 and one["done"] == 1 and np.array_equal(one["match"], m) and np.array_equal(bits(one["gap"]), bits(gp))
    assert np.array_equal(one["mt"][0], res["mt"][0]) and np.array_equal(bits(one["gt"][0]), bits(res["gt"][0]))
    # a seed given in another order is the same seed (the pairs go into Z in ascending a)
    if len(seedA) > 1:
        rev = run_ipa(g, ctx, P, Zfix, seedA[::-1].copy(), seedB[::-1].copy(), max_rounds=1)
        assert rev["rc"] == 0 and np.array_equal(rev["match"], m) and np.array_equal(bits(rev["gap"]), bits(gp))


# ---- determinism --------------------------------------------------------------------------------------------------------------------------
def test_determinism(g, ctx):
    P = pools(21, 60, 30)
    Zfix, seedA, seedB = im.variant(P, "both")
    first = run_ipa(g, ctx, P, Zfix, seedA, seedB)
    assert first["rc"] == 0 and first["done"] >= 3

    def same(r):
        assert r["rc"] == 0 and r["done"] == first["done"]
        assert np.array_equal(r["match"], first["match"]) and np.array_equal(bits(r["gap"]), bits(first["gap"]))
        cols = [F[k] for k in ("M_train", "candidates", "n_sel", "n_changed", "Meff", "theta", "logdet", "cost")]
        assert np.array_equal(bits(r["rounds"][:, cols]), bits(first["rounds"][:, cols]))

    again = run_ipa(g, ctx, P, Zfix, seedA, seedB)
    same(again)
    assert np.array_equal(again["mt"], first["mt"]) and np.array_equal(bits(again["gt"]), bits(first["gt"]))
    off = run_ipa(g, ctx, P, Zfix, seedA, seedB, traces=False)
    same(off)
    assert np.all(off["mt"] == 77) and np.all(off["gt"] == 7.5)
    for chunk in (128, 333):   # (K_A = 162: the second chunk of 128 starts inside a species)
        c = g.Context(0).set_options(PAIR_CHUNK=chunk)
        try:
            r = run_ipa(g, c, P, Zfix, seedA, seedB)
            same(r)
            assert np.array_equal(r["mt"], first["mt"]) and np.array_equal(bits(r["gt"]), bits(first["gt"]))
        finally:
            c.close()
    # the stage times: reported by a timed context (the default), 0 otherwise
    ms = [F[k] for k in ("ms_fit", "ms_match", "ms_select")]
    assert np.all(first["rounds"][:first["done"], ms] > 0.0)
    c = g.Context(0)
    try:
        c.set_timing(False)
        r = run_ipa(g, c, P, Zfix, seedA, seedB, max_rounds=2)
        same_bits = [F[k] for k in ("n_sel", "logdet", "cost")]
        assert r["rc"] == 0 and np.all(r["rounds"][:2, ms] == 0.0) and np.array_equal(bits(r["rounds"][:2, same_bits]), bits(first["rounds"][:2, same_bits]))
    finally:
        c.close()


# ---- the collect-time branches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1)])
def test_the_loop_through_the_collect_time_branches(g, option, value, refined):
    P = pools(21, 60, 30)
    Zfix, seedA, seedB = im.variant(P, "both")
    c = g.Context(0)
    try:
        c.set_option(option, value)
        res = run_ipa(g, c, P, Zfix, seedA, seedB, max_rounds=3)
        assert res["rc"] == 0 and res["done"] == 3 and res["st"].refined == refined
        Z = im.seed_alignment(Zfix, P["XA"], P["XB"], seedA, seedB)
        for r in range(1, 4):   # its own host-driven reproduction under the same option
            m, gp, _, logdet, st = partner_match(g, c, P, Z)
            assert st.refined == refined
            assert np.array_equal(m, res["mt"][r - 1]) and np.array_equal(bits(gp), bits(res["gt"][r - 1])), r
            assert bits(res["rounds"][r - 1, F["logdet"]]) == bits(logdet)
            Z = im.next_training_set(Zfix, P["XA"], P["XB"], m, gp, r * im.N_INC)[0]
    finally:
        c.close()


# ---- against the model -----------------------------------------------------------------------------------------------------------------------
def test_natives_per_round_equal_the_models_record(g, ctx):
    """asserted because tests/test_ipa_cpu.py has held every round's margins of this case against the bars"""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "ipa_family.json")))
    case = rec["case"]
    P = pools(case["q"], case["N"], case["split"])
    Zfix, seedA, seedB = im.variant(P, case["variant"])
    res = run_ipa(g, ctx, P, Zfix, seedA, seedB, n_inc=case["n_inc"], max_rounds=case["max_rounds"], pc=case["pseudocount"])
    assert res["rc"] == 0 and res["done"] == len(rec["rounds"])
    got = [im.natives(P, res["mt"][r]) for r in range(res["done"])]
    print("natives per round: device", got, "model", [rd["natives"] for rd in rec["rounds"]])
    assert got == [rd["natives"] for rd in rec["rounds"]]
    for r, rd in enumerate(rec["rounds"]):
        row = res["rounds"][r]
        assert (row[F["M_train"]], row[F["candidates"]], row[F["n_sel"]], row[F["n_changed"]]) == \
            (rd["M_train"], rd["candidates"], rd["n_sel"], rd["n_changed"]), (r, row, rd)


# ---- the Python entry ------------------------------------------------------------------------------------------------------------------------
def test_python_entry_takes_labels_in_any_order(g, ctx, tmp_path):
    from gaussdca.jl_amd.synth import write_fasta

    P = pools(21, 60, 30)
    labels_a, labels_b = np.repeat(np.arange(len(P["offA"]) - 1), np.diff(P["offA"])), np.repeat(np.arange(len(P["offB"]) - 1), np.diff(P["offB"]))
    rng = np.random.default_rng(4)
    sa, sb = rng.permutation(len(labels_a)), rng.permutation(len(labels_b))
    YA, YB, la, lb = P["XA"][:, sa], P["XB"][:, sb], labels_a[sa] * 3 - 5, labels_b[sb] * 3 - 5
    known = str(tmp_path / "known.fasta")
    write_fasta(known, np.ascontiguousarray(P["Zfix"].T))
    match, gap, rounds = g.gDCA_partner_ipa(YA, YB, la, lb, known_pairs=known, seed="singletons", n_inc=im.N_INC, max_rounds=4, pseudocount=PC,
                                            max_gap_fraction=1.0, q=21, ctx=ctx)
    # the same pools sorted by species the wrapper's way (stable: the caller's order inside a species), through the C-ABI
    perm_a, perm_b, offA, offB, _ = g.species_blocks(la, lb)
    assert np.array_equal(offA, P["offA"]) and np.array_equal(offB, P["offB"])
    Ps = dict(P, XA=np.asfortranarray(YA[:, perm_a]), XB=np.asfortranarray(YB[:, perm_b]))
    ref = run_ipa(g, ctx, Ps, P["Zfix"], P["seedA"], P["seedB"], max_rounds=4)
    assert ref["rc"] == 0 and len(rounds) == ref["done"] == 4 and g.gdca.last_stats["M"] == rounds[-1]["M_train"]
    m_want, g_want = np.empty_like(ref["match"]), np.empty_like(ref["gap"])
    m_want[perm_a] = np.where(ref["match"] >= 0, perm_b[np.maximum(ref["match"], 0)], -1)
    g_want[perm_a] = ref["gap"]
    assert np.array_equal(match, m_want) and np.array_equal(bits(gap), bits(g_want))
    assert np.all(la[match >= 0] == lb[match[match >= 0]])   # inside the species
    assert [r["n_sel"] for r in rounds] == ref["rounds"][:4, F["n_sel"]].tolist()
    # an explicit seed, in the caller's indices
    pairs = [(int(perm_a[a]), int(perm_b[b])) for a, b in zip(P["seedA"], P["seedB"])]
    m2, g2, r2 = g.gDCA_partner_ipa(YA, YB, la, lb, known_pairs=known, seed=pairs, n_inc=im.N_INC, max_rounds=4, pseudocount=PC,
                                    max_gap_fraction=1.0, q=21, ctx=ctx)
    assert np.array_equal(m2, match) and np.array_equal(bits(g2), bits(gap))
    with pytest.raises(g.ArgumentError):
        g.gDCA_partner_ipa(YA, YB, la, lb, seed=[], ctx=ctx)                       # nothing to fit on
    with pytest.raises(g.ArgumentError):
        g.gDCA_partner_ipa(YA, YB, la, lb, seed=[(0, 0), (0, 1)], q=21, ctx=ctx)   # an a twice (or across species)
    with pytest.raises(g.ArgumentError):
        g.gDCA_partner_ipa(YA, YB, la[:-1], lb, ctx=ctx)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_alone(g, ctx):
    P = pools(5, 7, 3)
    p, EINVAL = g._lib._p, g._lib.GDCA_EINVAL
    Zfix, seedA, seedB = P["Zfix"], P["seedA"], P["seedB"]
    KA, KB = P["XA"].shape[1], P["XB"].shape[1]

    def refused(zfix=Zfix, sa=seedA, sb=seedB, **over):
        r = run_ipa(g, ctx, P, zfix, np.asarray(sa, dtype=np.int32), np.asarray(sb, dtype=np.int32), **over)
        untouched = np.all(r["match"] == 77) and np.all(r["gap"] == 7.5) and np.all(r["mt"] == 77) and np.all(r["gt"] == 7.5) and \
            np.all(r["rounds"] == -9.0) and r["done"] == -5
        return r["rc"] == EINVAL and untouched

    none = np.empty(0, dtype=np.int32)
    # the checks of gdca_run_partner_match
    bad = P["offA"].copy()
    bad[4], bad[5] = bad[5], bad[4]
    short = P["offA"].copy()
    short[-1] -= 1
    assert refused(offA=p(bad)) and refused(offA=p(short)) and refused(S=0) and refused(offB=None) and refused(what=2)
    assert refused(split=0) and refused(split=7) and refused(q=1) and refused(q=32) and refused(KA=0) and refused(prm=None) and refused(XA=None)
    assert refused(match=None)
    assert refused(pc=1.5)
    # the loop's own
    assert refused(zfix=None, sa=none, sb=none)                                   # Mfix + n_seed < 1
    assert refused(sa=[KA], sb=[0]) and refused(sa=[0], sb=[-1]) and refused(sa=[-1], sb=[0]) and refused(sa=[0], sb=[KB])   # outside its pool
    a3, b3 = int(P["offA"][3]), int(P["offB"][4])
    assert refused(sa=[a3], sb=[b3])                                              # across two species
    a5, b5 = int(P["offA"][5]), int(P["offB"][5])
    assert refused(sa=[a5, a5], sb=[b5, b5 + 1]) and refused(sa=[a5, a5 + 1], sb=[b5, b5])   # an a twice, a b twice
    assert refused(n_inc=0) and refused(max_rounds=0) and refused(n_inc=-3)
    assert refused(Mfix=2**31 - 100)                                              # Mfix + K_A beyond an int32
    assert refused(Mfix=-1) and refused(Zfix_ptr=None)                               # (Mfix > 0 without a Zfix)
    # a bad symbol in a pool: found on the device before the first round
    YB = P["XB"].copy(order="F")
    YB[1, 100] = P["q"] + 1
    r = run_ipa(g, ctx, P, Zfix, seedA, seedB, XB=p(YB))
    assert r["rc"] == EINVAL and r["done"] == 0 and np.all(r["match"] == 77) and np.all(r["mt"] == 77) and np.all(r["rounds"] == -9.0)
    # the context is usable afterwards, and the seed may lie in any species with both sides
    ok = run_ipa(g, ctx, P, Zfix, [a5, a5 + 1], [b5 + 1, b5], max_rounds=2)
    assert ok["rc"] == 0 and ok["done"] == 2
