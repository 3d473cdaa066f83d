"""Iterative partner matching without a GPU: the selection rule, the stop rule, the binding, the kernels' resources, and the model loop
(tests/ipa_model.py) through the oracle's fit on the paired family the GPU tests run on -- its natives per round and its margins are
recorded in tests/golden/ipa_family.json, and every margin is held against the bars of ipa_model's docstring HERE, so that
tests/test_gpu_ipa.py may assert the device's natives per round against the record.

    python tests/test_ipa_cpu.py        writes tests/golden/ipa_family.json again (the model alone; no GPU)"""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import energy_model as em  # noqa: E402
import ipa_model as im  # noqa: E402
import pair_energy_model as pm  # noqa: E402
import partner_model as pt  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ipa_family.json")
# The recorded case: the listed family (paired_family's default seed) at q = 21, N = 60, split = 30, Zfix of 40 pairs and an empty seed,
# pseudocount 0.5.  Chosen on the model alone: of the three variants at pseudocount 0.5 and 0.8 this one keeps every round's margins
# furthest above the bars (least second-best margin minus its bar 0.11, least selection margin 0.16 against a bar of 0.004); "both" at
# 0.5 misses the assignment's bar in round 5 by 0.005 and is therefore not the one compared.
CASE = dict(q=21, N=60, split=30, variant="fix", pseudocount=0.5, n_inc=im.N_INC, max_rounds=12)


# ---- the selection rule ----------------------------------------------------------------------------------------------------------------
def test_selection_rule_on_handcrafted_vectors():
    inf = np.inf
    #                 a: 0     1     2     3    4     5     6    7     8     9
    gap = np.array([1.5, -0.0, inf, 0.0, -2.0, 1.5, 9.0, inf, -0.5, 0.0])
    match = np.array([4, 2, 7, 1, 0, 3, -1, 9, 8, 5])   # a = 6 (the largest finite gap) is unmatched
    order = [2, 7, 0, 5, 3, 9, 1, 8, 4]               # +inf first (ties by a), 1.5 twice by a, 0.0 twice by a before -0.0, negatives last
    for n_take in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, -3):
        sel, n = im.select(match, gap, n_take)
        want = sorted(order[:max(n_take, 0)])
        assert n == len(want) and sel[:n].tolist() == want and np.all(sel[n:] == -1) and len(sel) == 10, n_take
        assert 6 not in sel[:n]
    # -0.0 after 0.0 whatever their places; a NaN (the ranking's order: first of all)
    sel, n = im.select([0, 0, 0], [-0.0, 0.0, 0.0], 2)
    assert sel.tolist() == [1, 2, -1] and n == 2
    sel, n = im.select([0, 0, 0], [np.inf, np.nan, 5.0], 1)
    assert sel.tolist() == [1, -1, -1]
    # all unmatched
    sel, n = im.select([-1, -1], [3.0, 4.0], 2)
    assert n == 0 and sel.tolist() == [-1, -1]
    # the key is the host ranking's: ascending keys = its order
    vals = np.array([np.nan, np.inf, 3.0, 0.0, -0.0, -1.0, -np.inf])
    assert np.all(np.diff(im.rank_key(vals).astype(object)) > 0)
    # margins: the last selected against the first rejected
    assert im.selection_margin(match, gap, 3) == 0.0 and im.selection_margin(match, gap, 4) == 1.5
    assert im.selection_margin(match, gap, 1) == inf and im.selection_margin(match, gap, 9) == inf and im.selection_margin(match, gap, 2) == inf


def test_concat_and_next_training_set():
    rng = np.random.default_rng(0)
    XA, XB = rng.integers(1, 6, size=(3, 7)).astype(np.int8), rng.integers(1, 6, size=(4, 9)).astype(np.int8)
    Z = im.concat(XA, XB, [5, 0], [8, 2])
    assert Z.shape == (7, 2) and Z.flags.f_contiguous and Z.dtype == np.int8
    assert np.array_equal(Z[:3, 0], XA[:, 5]) and np.array_equal(Z[3:, 0], XB[:, 8]) and np.array_equal(Z[:, 1], np.concatenate([XA[:, 0], XB[:, 2]]))
    match, gap = np.array([3, -1, 0, 8, 1, 2, 5]), np.array([0.5, 9.0, 2.0, 0.1, 0.7, np.inf, -1.0])
    Zfix = rng.integers(1, 6, size=(7, 2)).astype(np.int8)
    Zn, sel, n = im.next_training_set(Zfix, XA, XB, match, gap, 3)
    assert n == 3 and sel.tolist() == [2, 4, 5, -1, -1, -1, -1]   # inf, 2.0, 0.7 -- in ascending a
    assert np.array_equal(Zn[:, :2], Zfix) and np.array_equal(Zn[:, 2:], im.concat(XA, XB, [2, 4, 5], [0, 1, 2]))
    assert im.next_training_set(None, XA, XB, match, gap, 1)[0].shape == (7, 1)


# ---- the stop rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,n_inc", [(1, 1), (5, 16), (16, 16), (17, 16), (33, 8), (40, 7)])
def test_stop_rule_and_round_count_on_a_stub_matcher(P, n_inc):
    KA = P + 3
    rng = np.random.default_rng(P)
    match = np.concatenate([np.arange(P), [-1, -1, -1]])[rng.permutation(KA)]
    gap = rng.integers(0, 4, size=KA).astype(np.float64)    # ties are the rule
    XA, XB = np.ones((1, KA), dtype=np.int8), np.ones((1, KA), dtype=np.int8)
    calls = []

    def stub(Z):
        calls.append(Z.shape[1])
        return match, gap

    rounds = im.loop(stub, np.ones((2, 1), dtype=np.int8), XA, XB, [], [], n_inc, 1000)
    assert len(rounds) == math.ceil(P / n_inc) + 1 == len(calls)
    assert calls == [1] + [1 + min(r * n_inc, P) for r in range(1, len(rounds))]   # Zfix and r n_inc pairs, afresh every round
    assert [r["n_sel"] for r in rounds] == [min(r * n_inc, P) for r in range(1, len(rounds) + 1)]
    assert rounds[0]["n_changed"] == P and all(r["n_changed"] == 0 for r in rounds[1:]) and all(r["candidates"] == P for r in rounds)
    # max_rounds cuts it short; without Zfix a round that selects nothing ends it
    assert len(im.loop(stub, np.ones((2, 1), dtype=np.int8), XA, XB, [], [], n_inc, 1)) == 1
    none = im.loop(lambda Z: (np.full(KA, -1), gap), None, XA, XB, [0], [0], n_inc, 9)
    assert len(none) == 1 and none[0]["n_sel"] == 0


# ---- the binding and the header ---------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gdca_select_confident_dev", "gdca_select_confident", "gdca_concat_pairs_dev", "gdca_concat_pairs", "gdca_run_partner_ipa_dev",
               "gdca_run_partner_ipa")


def test_binding_and_header_declare_the_loop():
    from gaussdca.jl_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "gdca.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert len(_lib.SYMBOLS["gdca_run_partner_ipa"][1]) == len(_lib.SYMBOLS["gdca_run_partner_ipa_dev"][1]) == 27
    m = re.search(r"#define GDCA_IPA_FIELDS (\d+)", hdr)
    assert m and int(m.group(1)) == len(_lib.IPA_FIELDS) == len(im.IPA_FIELDS) == 12
    enum = re.search(r"enum \{\s*(GDCA_IPA_M_TRAIN.*?)\};", hdr, flags=re.S).group(1)
    names = [x.split("=")[0].strip().replace("GDCA_IPA_", "").lower() for x in enum.split(",")]
    assert names == [f.lower() for f in _lib.IPA_FIELDS] and tuple(_lib.IPA_FIELDS) == im.IPA_FIELDS
    assert re.search(r"#define GDCA_VERSION_MINOR 6\b", hdr)   # (only functions are added)
    import gaussdca.jl_amd as g

    assert callable(g.gDCA_partner_ipa) and all(hasattr(g.Context, a) for a in ("select_confident", "concat_pairs", "run_partner_ipa_ptr",
                                                                                "run_partner_ipa_dev"))
    lib = _lib.load()   # (binds every symbol: the library exports them)
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)


def test_ipa_kernels_run_without_scratch(tmp_path):
    from gdca_testutil import HIPCC, compiler_report

    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    compiler_report(tmp_path, "k_ipa.hip", kernels=["k_ipa_keys", "k_ipa_flag", "k_ipa_compact", "k_ipa_concat", "k_ipa_round", "k_ipa_publish"])


# ---- the model loop on the GPU tests' family ---------------------------------------------------------------------------------------------
def model_rounds(case=CASE):
    """the loop through the oracle's fit, pair_energy_model and scipy's assignment -> one record a round"""
    q, pc = case["q"], case["pseudocount"]
    P = im.pools(q, case["N"], case["split"])
    Zfix, seedA, seedB = im.variant(P, case["variant"])
    offA, offB = P["offA"], P["offB"]
    S = len(offA) - 1
    notes = []

    def fit_and_match(Z):
        mJ, Pi = em.model_from_Z(np.ascontiguousarray(Z.T), q, pc)
        E = pm.pair_energy(mJ, Pi, P["XA"], P["XB"], q)[0]
        blocks = pt.cut_blocks(E, offA, offB)
        emax = max(float(np.abs(b).max()) for b in blocks if b.size)
        ebar = (1e-6 + 1e-9) * emax
        match, gap = np.full(offA[-1], -1, dtype=np.int64), np.zeros(offA[-1])
        slack = np.inf   # least (second-best margin - bar) over the species
        margin = np.inf
        for s in range(S):
            b = blocks[s]
            if not b.size:
                continue
            m = pt.assign_scipy(b)[0]
            match[offA[s]:offA[s + 1]] = np.where(m >= 0, m + offB[s], -1)
            gap[offA[s]:offA[s + 1]] = pt.gap_of(b, m)
            sb = pt.second_best_margin(b)
            margin = min(margin, sb)
            slack = min(slack, sb - (pt.solver_bar(b) + 2 * max(b.shape) * ebar))
        notes.append(dict(ebar=ebar, second_best_margin=margin, assign_slack=slack))
        return match, gap

    rounds = im.loop(fit_and_match, Zfix, P["XA"], P["XB"], seedA, seedB, case["n_inc"], case["max_rounds"])
    out = []
    for r, (rd, nt) in enumerate(zip(rounds, notes), 1):
        out.append(dict(round=r, M_train=int(rd["Z"].shape[1]), candidates=rd["candidates"], n_sel=rd["n_sel"], n_changed=rd["n_changed"],
                        natives=im.natives(P, rd["match"]), selection_margin=im.selection_margin(rd["match"], rd["gap"], r * case["n_inc"]),
                        selection_bar=4 * nt["ebar"], second_best_margin=nt["second_best_margin"], assign_slack=nt["assign_slack"]))
    return out


@pytest.fixture(scope="module")
def modelled():
    return model_rounds()


def test_model_loop_margins(modelled):
    """every round's margins exceed the bars (ipa_model's docstring): only then does the GPU comparison mean anything"""
    for rd in modelled:
        print("round %2d: M %3d, selected %3d of %3d, changed %3d, natives %3d; selection margin %.3g (bar %.3g), second-best margin %.3g (slack %.3g)"
              % (rd["round"], rd["M_train"], rd["n_sel"], rd["candidates"], rd["n_changed"], rd["natives"], rd["selection_margin"],
                 rd["selection_bar"], rd["second_best_margin"], rd["assign_slack"]))
    assert len(modelled) == math.ceil(modelled[0]["candidates"] / CASE["n_inc"]) + 1
    for rd in modelled:
        assert rd["selection_margin"] > rd["selection_bar"], rd
        assert rd["assign_slack"] > 0.0, rd
    assert modelled[-1]["natives"] > modelled[0]["natives"]   # the loop does what it is for


def test_model_loop_equals_the_record(modelled):
    rec = json.load(open(GOLDEN))
    assert rec["case"] == CASE and len(rec["rounds"]) == len(modelled)
    for a, b in zip(rec["rounds"], modelled):
        for k in ("round", "M_train", "candidates", "n_sel", "n_changed", "natives"):
            assert a[k] == b[k], (k, a, b)
        for k in ("selection_margin", "second_best_margin"):
            assert (a[k] == b[k]) or abs(a[k] - b[k]) <= 1e-6 * abs(b[k]), (k, a, b)


if __name__ == "__main__":
    rounds = model_rounds()
    for rd in rounds:
        print(rd)
    with open(GOLDEN, "w") as f:
        json.dump(dict(case=CASE, rounds=rounds), f, indent=1)   # (an infinite margin is written as Infinity, which json.load reads back)
        f.write("\n")
