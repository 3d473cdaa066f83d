"""The pair log-odds stated in numpy (tests/logodds_model.py) held against independent statements of itself, the recorded
illustration, and the new entry points' place in the C-ABI.  No GPU: the device is held to this model by tests/test_gpu_logodds.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import logodds_model as lo
import pair_energy_model as pm
from gdca_testutil import random_msa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussdca.jl_amd", "libgdca.so")

NEW_SYMBOLS = ["gdca_pair_logodds", "gdca_pair_logodds_dev", "gdca_pair_logodds_blocked", "gdca_pair_logodds_blocked_dev",
               "gdca_run_pair_logodds", "gdca_run_pair_logodds_dev", "gdca_run_partner_logodds", "gdca_run_partner_logodds_dev"]

# a family small enough for dense statements: n = 44, n_A = 16
Q, N, SPLIT, M = 5, 11, 4, 300


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(31)
    Zo = random_msa(rng, M, N, q=Q)
    XA, XB = pm.mixed_halves(rng, Zo, Q, SPLIT, 9, 7)
    return Zo, XA, XB


def _logpdf(x, mean, cov):
    """log N(x; mean, cov): scipy's, or -- without scipy -- the dense float64 quadratic form and slogdet"""
    try:
        from scipy.stats import multivariate_normal

        return multivariate_normal(mean=mean, cov=cov).logpdf(x)
    except ImportError:
        d = np.asarray(x) - mean
        quad = np.einsum("ki,ki->k", d @ np.linalg.inv(cov), d)
        return -0.5 * (quad + len(mean) * np.log(2 * np.pi) + np.linalg.slogdet(cov)[1])


def _dense_logodds(m, XA, XB):
    """L[a, b] = logpdf_AB(a (+) b) - logpdf_A(a) - logpdf_B(b) on the oracle's C and Pi"""
    import energy_model as em

    KA, KB = XA.shape[1], XB.shape[1]
    cat = em.one_hot(pm.concatenations(XA, XB), m.q)  # row a + KA b
    lab = _logpdf(cat, m.Pi, m.C).reshape(KB, KA).T
    la = _logpdf(em.one_hot(XA, m.q), m.PiA, m.CA)
    lb = _logpdf(em.one_hot(XB, m.q), m.PiB, m.CB)
    return lab - la[:, None] - lb[None, :]


def test_the_model_is_the_difference_of_three_log_densities(small):
    Zo, XA, XB = small
    m = lo.Model(Zo, Q, 0.5, SPLIT)
    p = m.parts(XA, XB)
    L_dense = _dense_logodds(m, XA, XB)
    frac = np.abs(p["L"] - L_dense) / p["bar"]
    print("model vs the three log densities: max err / bar %.3g (max bar %.3g, I = %.6g)" % (float(frac.max()), float(p["bar"].max()), m.I))
    assert np.all(frac <= 1.0)
    assert m.I > 0 and abs(m.I - lo.information_f64(m.ld, m.ldA, m.ldB)) <= m.bar_I
    assert np.array_equal(lo.combine_f64(p["EmA"], p["EmB"], p["E"], m.I), p["L"])


def test_pseudocount_one_has_no_information(small):
    """C is block diagonal to rounding: the joint model is the product of its marginals"""
    Zo, XA, XB = small
    m = lo.Model(Zo, Q, 1.0, SPLIT)
    p = m.parts(XA, XB)
    print("pseudocount 1: |I| = %.3g (bar %.3g), max |L| / bar = %.3g" % (abs(m.I), m.bar_I, float((np.abs(p["L"]) / p["bar"]).max())))
    assert abs(m.I) <= m.bar_I
    assert np.all(np.abs(p["L"]) <= p["bar"])


def test_swapping_the_halves_transposes_the_matrix(small):
    Zo, XA, XB = small
    m = lo.Model(Zo, Q, 0.5, SPLIT)
    ms = lo.Model(lo.swapped(Zo, SPLIT), Q, 0.5, N - SPLIT)
    p, ps = m.parts(XA, XB), ms.parts(XB, XA)
    both = p["bar"] + ps["bar"].T
    frac = np.abs(p["L"] - ps["L"].T) / both
    print("halves swapped: max |L - L'^T| / (sum of the two bars) %.3g, |I - I'| = %.3g" % (float(frac.max()), abs(m.I - ms.I)))
    assert np.all(frac <= 1.0)
    assert abs(m.I - ms.I) <= m.bar_I + ms.bar_I


def test_the_recorded_illustration():
    """tests/golden/logodds_family.json: the figures of the recorded illustration, recomputed by the model"""
    with open(lo.GOLDEN) as f:
        gold = json.load(f)
    rec = lo.family_record()
    assert gold["command"] == lo.GOLDEN_COMMAND and gold["family"] == rec["family"]
    for key in ("native_fraction_E", "native_fraction_L", "natives_by_assignment"):
        assert gold[key] == rec[key], key
    bar_I = lo.family_model()[0].bar_I
    assert abs(gold["information"] - rec["information"]) <= bar_I
    assert np.allclose(gold["logdet"], rec["logdet"], rtol=0, atol=2 * bar_I)
    for key in ("mean_L_native", "mean_L_nonnative"):
        assert abs(gold[key] - rec[key]) <= rec["max_bar"], key
    assert np.isclose(gold["min_row_margin_over_bar"], rec["min_row_margin_over_bar"], rtol=1e-3)
    assert [s["size"] for s in gold["species"]] == list(lo.SPECIES_SIZES)
    for sg, sr in zip(gold["species"], rec["species"]):
        assert sg["decided"] and sr["decided"] and sg["natives"] == sr["natives"]  # every species' margin exceeds twice its bar
    # the point of the score: the log-odds finds the native partner far more often than the joint energy does
    assert rec["native_fraction_L"] > 2 * rec["native_fraction_E"]
    assert rec["mean_L_native"] > 0 > rec["mean_L_nonnative"] and rec["information"] > 0
    print("row-best native: E %.3f, L %.3f; I = %.4f nats; natives by assignment on L: %d of 40" %
          (rec["native_fraction_E"], rec["native_fraction_L"], rec["information"], rec["natives_by_assignment"]))


def test_pseudocount_one_on_the_family():
    m, XA, XB, p = lo.family_model(1.0)
    assert abs(m.I) < 1e-11 and np.all(np.abs(p["L"]) < 1e-11)


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------------
_CTYPES = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}


def _header_prototypes():
    """{name: [argument types as the header spells them]} of include/gdca.h"""
    src = open(os.path.join(ROOT, "include", "gdca.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"gdca_status\s+(gdca_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [re.sub(r"\s*\b\w+$", "", a.strip()).strip() for a in args.split(",")]
    return out


def test_the_new_symbols_are_exported_and_bound_as_the_header_declares_them():
    from gaussdca.jl_amd import _lib

    assert os.path.exists(LIB), "libgdca.so has not been built"
    lib = ctypes.CDLL(LIB)
    protos = _header_prototypes()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in protos and name in _lib.SYMBOLS, name
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int
        decl = protos[name]
        assert len(decl) == len(args), (name, len(decl), len(args))
        for i, (c, py) in enumerate(zip(decl, args)):
            if c == "gdca_ctx *":
                want = _lib._ctx
            elif c == "const gdca_params *":
                want = ctypes.POINTER(_lib.Params)
            elif c == "gdca_stats *":
                want = ctypes.POINTER(_lib.Stats)
            elif c.endswith("*"):
                want = ctypes.c_void_p
            else:
                want = _CTYPES[c]
            assert py is want or py == want, (name, i, c, py)
    assert len(_lib.LOGODDS_FIELDS) == 8
    src = open(os.path.join(ROOT, "include", "gdca.h")).read()
    assert re.search(r"#define GDCA_LOGODDS_FIELDS 8\b", src)
    enum = re.search(r"enum \{\s*(GDCA_LOGODDS_LOGDET = 0[^}]*)\}", src).group(1)
    names = [e.strip().split(" ")[0] for e in enum.split(",")]
    assert [n[len("GDCA_LOGODDS_"):].lower() for n in names] == [f.lower() for f in _lib.LOGODDS_FIELDS]
