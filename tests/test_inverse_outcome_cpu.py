"""What happens after an SPD inverse has run, and how a call ends (csrc/gdca_inverse_outcome.h), on the CPU: the header
is plain C++ shared by gdca_api.hip and this test, which compiles it alone with the host compiler and calls it through ctypes.

The decisions and the verdict are checked against the rules as they stood before the header existed, restated below in Python from
that code: gdca_run_collect's loop and ifs for a fused run; operator_norms_and_refine, operator_fallback, operator_inverse_retry and
the ends of gdca_spd_inverse_dev / gdca_spd_inverse_batch_dev for an operator-level inverse; symbols_ok and sequences_checked."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussdca.jl_amd", "csrc")
WATCHDOG = -2**31
OK, EINVAL, ENOTPD, EHIP, ENOCONV = 0, 1, 2, 3, 5
RUN, OPERATOR = 0, 1
ENDS_RUN, ENDS_INVERSE, ENDS_READOUT, ENDS_FRONT = 0, 1, 2, 3
RETRIES = 2        # option SWEEP_RETRIES' default
REFINE_COND = 1e6  # option REFINE_COND's default


class State(ctypes.Structure):
    _fields_ = [("form", ctypes.c_int), ("info", ctypes.c_int), ("bad_symbol", ctypes.c_int),
                ("inv_norm1", ctypes.c_double), ("mat_norm1", ctypes.c_double), ("ns_resid", ctypes.c_double), ("pi_max", ctypes.c_double),
                ("pc", ctypes.c_double), ("N", ctypes.c_int), ("q", ctypes.c_int), ("refine", ctypes.c_int), ("cholesky", ctypes.c_int),
                ("refine_cond", ctypes.c_double), ("attempt", ctypes.c_int), ("retries", ctypes.c_int)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    d = tmp_path_factory.mktemp("outcome")
    src = d / "outcome.cpp"
    src.write_text('#include "gdca_inverse_outcome.h"\n'
                   'static_assert(GDCA_BAD_ALIGNMENT == 1 && GDCA_BAD_WEIGHT == 2 && GDCA_BAD_SEQUENCE == 4 && GDCA_BAD_INDEX == 8 && GDCA_BAD_MUTANT == 16, "");\n'
                   'extern "C" int watchdog(void) { return GDCA_INFO_WATCHDOG; }\n'
                   'extern "C" int state_bytes(void) { return (int)sizeof(gdca_inverse_state); }\n'
                   'extern "C" int retry_due(const gdca_inverse_state *s) { return gdca_retry_due(*s); }\n'
                   'extern "C" int norm_due(const gdca_inverse_state *s) { return gdca_norm_due(*s); }\n'
                   'extern "C" int wants_refinement(const gdca_inverse_state *s) { return gdca_wants_refinement(*s); }\n'
                   'extern "C" int refined_after_step(const gdca_inverse_state *s) { return gdca_refined_after_step(*s); }\n'
                   'extern "C" int wants_cholesky(const gdca_inverse_state *s, int refined) { return gdca_wants_cholesky(*s, refined); }\n'
                   'extern "C" double cond_bound(double m, double p, double pc, int q, int N) { return gdca_cond_bound(m, p, pc, q, N); }\n'
                   'extern "C" int norm1_settled(int N, int q, double pc, int refine, double cond) { return gdca_norm1_settled(N, q, pc, refine, cond); }\n'
                   'extern "C" int verdict(int kind, int bad, int info, int noconv, const char **text)\n'
                   '{ const gdca_verdict v = gdca_verdict_of(kind, bad, info, noconv); *text = v.text; return v.status; }\n'
                   'extern "C" int worse(int s0, const char *t0, int s1, const char *t1, const char **text)\n'
                   '{ const gdca_verdict v = gdca_worse_verdict(gdca_verdict{(gdca_status)s0, t0}, gdca_verdict{(gdca_status)s1, t1}); *text = v.text; return v.status; }\n')
    so = d / "outcome.so"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    sp = ctypes.POINTER(State)
    for name in ("retry_due", "norm_due", "wants_refinement", "refined_after_step"):
        getattr(lib, name).argtypes = [sp]
    lib.wants_cholesky.argtypes = [sp, ctypes.c_int]
    lib.cond_bound.restype = ctypes.c_double
    lib.cond_bound.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    lib.norm1_settled.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double]
    lib.verdict.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]
    lib.worse.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p)]
    assert lib.watchdog() == WATCHDOG and lib.state_bytes() == ctypes.sizeof(State)
    return lib


# ---- the rules as they stood, restated ---------------------------------------------------------------------------------------------
def old_cond_bound(mat_norm1, pi_max, pc, q, N):
    c1 = mat_norm1 if mat_norm1 > 0.0 else 2.0 * N * pi_max
    if not c1 > 0.0 or not pc > 0.0:
        return float("inf")
    return c1 * q * q / pc


def old_wants_refinement(info, refine, inv_norm1, mat_norm1, cond):
    if info != 0 or refine == 0:
        return False
    if refine == 1:
        return True
    if not inv_norm1 > 0.0:
        return False
    return inv_norm1 * (mat_norm1 if mat_norm1 > 0.0 else 1.0) > cond


def old_wants_cholesky(cholesky, bad, info, refined):
    if cholesky == 0 or bad or info == WATCHDOG:
        return False
    return cholesky == 2 or info > 0 or refined < 0


def old_walk(form, info, bad, refine, cholesky, norms, resid, attempt, a_priori, retries=RETRIES):
    """One visit of the old code with the scalars of an attempt that has just ended.  norms: (inv_norm1, mat_norm1) as a
    measurement would give them -- a fused run's mat_norm1 is its front end's and there in any case; resid: what a Newton-Schulz
    step would report (sc->ns_resid stays 0 where none runs); a_priori: a fused run's cond_bound.
    -> (another attempt, the norm is measured, the step runs, gdca_stats.refined [a run], the fallback runs)"""
    inv1, mat1 = norms
    if form == RUN:
        retry = info == WATCHDOG and not bad and attempt < retries
        if retry:
            return (True, None, None, None, None)
        measured = refine != 0 and info == 0 and not bad and (refine == 1 or a_priori > REFINE_COND)
        step = old_wants_refinement(info, refine, inv1 if measured else 0.0, mat1, REFINE_COND) and not bad
        refined = (1 if resid < 1.0 else -1) if step else 0
        fallback = old_wants_cholesky(cholesky, bad, info, refined)
        return (False, measured, step, 2 if fallback else refined, fallback)
    # an operator: operator_inverse_once measures, steps and falls back on every attempt, then operator_inverse_retry looks at info
    measured = refine != 0
    step = measured and old_wants_refinement(info, refine, inv1, mat1, REFINE_COND)
    ns_resid = resid if step else 0.0
    fallback = old_wants_cholesky(cholesky, bad, info, -1 if ns_resid >= 1.0 else 0)
    retry = info == WATCHDOG and attempt < retries
    return (retry, measured, step, None, fallback)


def new_walk(lib, form, info, bad, refine, cholesky, norms, resid, attempt, pc, N, q, pi_max, retries=RETRIES):
    """inverse_ladder's walk over the same visit, every decision the header's"""
    inv1, mat1 = norms
    run = form == RUN
    s = State(form, info, bad, 0.0, mat1 if run else 0.0, 0.0, pi_max, pc if run else 0.0, N if run else 0, q if run else 0, refine, cholesky,
              REFINE_COND, attempt, retries)
    ref = ctypes.byref(s)
    retry = bool(lib.retry_due(ref))
    if retry and run:
        return (True, None, None, None, None)
    measured = bool(lib.norm_due(ref))
    if measured:
        s.inv_norm1, s.mat_norm1 = inv1, mat1
    step = bool(lib.wants_refinement(ref))
    refined = 0
    if step:
        s.ns_resid = resid
        refined = lib.refined_after_step(ref)
    fallback = bool(lib.wants_cholesky(ref, refined))
    return (retry, measured, step, (2 if fallback else refined) if run else None, fallback)


INFOS = (0, 7, WATCHDOG)
NORMS = ((0.0, 0.0), (10.0, 50.0), (1e5, 50.0))  # not measured; kappa_1 = 500 below the threshold; 5e6 above it
RESIDS = (0.0, 0.5, 1.0, 2.0)


def test_the_ladder_decides_as_the_two_copies_did(lib):
    N, q, pc = 12, 21, 0.8
    # a run's a-priori bound below the threshold (the usual family) and beyond it (a front end that measured ||C||_1 = 5e4)
    fronts = ((0.0, 0.9), (5e4, 0.9))
    assert old_cond_bound(*fronts[0], pc, q, N) < REFINE_COND < old_cond_bound(*fronts[1], pc, q, N)
    seen = set()
    for form, info, bad, refine, cholesky, norms, resid, attempt in itertools.product(
            (RUN, OPERATOR), INFOS, range(32), (-1, 0, 1), (0, 1, 2), NORMS, RESIDS, range(RETRIES + 1)):
        for front_norm, pi_max in (fronts if form == RUN else fronts[:1]):
            nm = (norms[0], front_norm if form == RUN else norms[1])
            want = old_walk(form, info, bad, refine, cholesky, nm, resid, attempt, old_cond_bound(front_norm, pi_max, pc, q, N))
            got = new_walk(lib, form, info, bad, refine, cholesky, nm, resid, attempt, pc, N, q, pi_max)
            if form == OPERATOR and want[0]:
                # (the old operator walked the rest of a doomed attempt before it tried again; whether it tries again is the decision)
                assert got[0], (form, info, bad, refine, cholesky, nm, resid, attempt)
                continue
            assert got == want, (form, info, bad, refine, cholesky, nm, resid, attempt, front_norm, got, want)
            seen.add((form,) + got)
    # every rung was reached in both forms, and every value of `refined`
    for form in (RUN, OPERATOR):
        assert {(r, m, s, f) for fm, r, m, s, _, f in seen if fm == form} >= {(False, True, True, True), (False, True, True, False),
                                                                              (False, False, False, True), (False, False, False, False)}
    assert {r for fm, again, _, _, r, _ in seen if fm == RUN and not again} == {0, 1, -1, 2}
    assert any(fm == RUN and r for fm, r, *_ in seen)


def test_retries_run_out(lib):
    for form, retries, attempt in itertools.product((RUN, OPERATOR), range(4), range(5)):
        s = State(form, WATCHDOG, 0, 0.0, 0.0, 0.0, 0.0, 0.8, 12, 21, -1, 1, REFINE_COND, attempt, retries)
        assert bool(lib.retry_due(ctypes.byref(s))) == (attempt < retries)
        s.retries = 0  # (the first pass of the batch form: its further attempts come later, one by one)
        assert not lib.retry_due(ctypes.byref(s))


def test_the_a_priori_screen(lib):
    for mat_norm1, pi_max, pc, q, N in itertools.product((0.0, 64.0, 5e4), (0.0, 0.3, 1.0), (0.0, 1e-4, 0.2, 0.8, 1.0), (2, 21, 31), (1, 12, 500)):
        assert lib.cond_bound(mat_norm1, pi_max, pc, q, N) == old_cond_bound(mat_norm1, pi_max, pc, q, N)
    for N, q, pc, refine, cond in itertools.product((1, 12, 500, 5000), (2, 21), (0.0, 1e-4, 0.2, 0.8, 1.0), (-1, 0, 1), (1e3, 1e6, 1e9)):
        pi_cap = (1.0 - pc) + pc / q
        want = pc > 0.0 and 2.0 * N * pi_cap * q * q / pc <= cond and refine != 1
        assert bool(lib.norm1_settled(N, q, pc, refine, cond)) == want
        # where it is settled, no alignment's bound asks for a measurement (pi_max <= pi_cap)
        if want:
            assert old_cond_bound(0.0, pi_cap, pc, q, N) <= cond


# ---- the verdict -------------------------------------------------------------------------------------------------------------------
SEQ = b"sequences hold a symbol outside 1..q"
MUT = b"a double-mutant record is out of range"
ALN = b"alignment holds a symbol outside 1..q"
DOG = b"SPD inverse aborted: a dependency wait inside the sweep kernel timed out"
COV = b"covariance matrix is not positive definite"
MAT = b"matrix is not positive definite; Cholesky factorization failed"
DI = b"eigenvalue iteration of a DI block did not converge"


def old_verdict(kind, bad, info, noconv):
    if kind == ENDS_RUN:  # the end of gdca_run_collect
        if bad & 4:
            return EINVAL, SEQ
        if bad & 16:
            return EINVAL, MUT
        if bad:
            return EINVAL, ALN
        if info == WATCHDOG:
            return EHIP, DOG
        if info != 0:
            return ENOTPD, COV
        if noconv != 0:
            return ENOCONV, DI
    elif kind == ENDS_INVERSE:  # the end of gdca_spd_inverse_dev
        if info == WATCHDOG:
            return EHIP, DOG
        if info != 0:
            return ENOTPD, MAT
    elif kind == ENDS_READOUT:  # sequences_checked
        if bad & 16:
            return EINVAL, MUT
        if bad:
            return EINVAL, SEQ
    elif bad:  # symbols_ok
        return EINVAL, ALN
    return OK, None


def test_the_verdict_and_its_texts(lib):
    text = ctypes.c_char_p()
    for kind, bad, info, noconv in itertools.product((ENDS_RUN, ENDS_INVERSE, ENDS_READOUT, ENDS_FRONT), range(32), INFOS, (0, 3)):
        status = lib.verdict(kind, bad, info, noconv, ctypes.byref(text))
        assert (status, text.value) == old_verdict(kind, bad, info, noconv), (kind, bad, info, noconv)


def test_the_batch_reports_its_worst_member(lib):
    """the end of gdca_spd_inverse_batch_dev: a member the watchdog ended overrides whatever stands; else the first failure stays"""
    text = ctypes.c_char_p()
    members = [old_verdict(ENDS_INVERSE, 0, info, 0) for info in INFOS]
    for batch in itertools.product(members, repeat=3):
        want = (OK, None)
        for status, t in batch:
            if status == EHIP:
                want = (status, t)
            elif status != OK and want[0] == OK:
                want = (status, t)
        got = (OK, None)
        for status, t in batch:
            st = lib.worse(got[0], got[1], status, t, ctypes.byref(text))
            got = (st, text.value)
        assert got == want, batch
