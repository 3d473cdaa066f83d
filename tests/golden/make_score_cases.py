"""Regenerates tests/golden/score_cases.npz (see README.md): for every DI case of tests/score_model.py the expected N x N matrix
of the 40-digit model, the per-pair scale B of the error bar, and a SHA-256 of the input bytes.  Expectations only: the inputs are
rebuilt from their seeds by score_model.score_cases.  About a minute of mpmath.  Prints, per case, the error of the f64 oracle
against the model in the bar's unit, the value DI_C_MEASURED of score_model.py must hold, and for comparison the plain ratio
err / (s^2 u B^2), with nothing taken off, over the pairs whose B is at least 1."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import score_model as sm  # noqa: E402
from oracle import gdca_oracle as o  # noqa: E402

out = {}
worst = plain = 0.0
for name in sm.DI_CASES:
    c = sm.score_cases("di", name)
    s = c["q"] - 1
    DI, B = sm.di_model(c["mJ"], c["C"], c["q"])
    err = np.abs(o.compute_DI_gauss(c["mJ"], c["C"], c["q"]) - DI)
    units = sm.di_units(s, B, err).max()
    worst = max(worst, units)
    big = B >= 1.0
    if big.any():
        plain = max(plain, float((err[big] / (s * s * sm.U * B[big] ** 2)).max()))
    print("%-16s s %2d N %2d  oracle - model: max %.2e (%.2f of the log-sum term 4 s u), beyond it %.3g units of s^2 u B^2"
          % (name, s, c["N"], err.max(), err.max() / (4 * s * sm.U), units))
    out[name + ".DI"] = DI
    out[name + ".B"] = B
    out[name + ".sha256"] = np.array(sm.input_hash(c["mJ"], c["C"]))
print("DI_C_MEASURED = %.3g -> DI_C = %g" % (worst, max(8.0, 8.0 * worst)))
print("plain err / (s^2 u B^2) over the pairs with B >= 1: %.3g" % plain)
np.savez_compressed(os.path.join(HERE, "score_cases.npz"), **out)
