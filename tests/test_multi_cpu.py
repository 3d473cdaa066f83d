"""Several settings of one alignment in one call, the parts that need no GPU: the C-ABI's three entry points are declared, exported
and bound; gDCA_multi checks every setting with check_arguments' own messages before it touches a device (and, without one, raises
like gDCA); the kernel that builds a covariance from the stored tallies compiles without scratch."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdca_run_multi", "gdca_run_multi_dev", "gdca_run_ranked_multi")
SMALL = os.path.join(ROOT, "tests", "golden", "reference", "small.fasta.gz")


@pytest.fixture(scope="module")
def g():
    import gaussdca.jl_amd as g

    if not os.path.exists(g._lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "gaussdca.jl_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    return g


def test_the_three_entry_points_are_declared_exported_and_bound(g):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdca.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bgdca_status\s+%s\s*\(" % n, src), n
        assert n in g._lib.SYMBOLS
        assert hasattr(ctypes.CDLL(g._lib.LIB_PATH), n), n
    assert re.search(r"#define GDCA_MULTI_MAX 16\b", src) and g._lib.MULTI_MAX == 16
    lib = g.load()
    # a null context is refused before anything else (no device needed)
    prm, K = g._lib._multi_params([(0.8, 0), (0.2, 1)], -1.0, True)
    assert lib.gdca_run_multi(None, None, 10, 10, 21, prm, K, None, None) == g._lib.GDCA_EINVAL
    assert lib.gdca_run_ranked_multi(None, None, 10, 10, 21, prm, K, 5, None, None, None, None) == g._lib.GDCA_EINVAL


@pytest.mark.parametrize("settings,bad", [
    ([(0.8, ":frob"), (1.5, ":DI")], (1.5, ":DI")),
    ([(0.8, ":frob"), (-0.1, "frob")], (-0.1, "frob")),
    ([(0.2, ":plm")], (0.2, ":plm")),
    ([(0.8, "frob"), {"pseudocount": 0.2, "score": "mi"}], (0.2, "mi")),
])
def test_settings_are_checked_with_check_arguments_messages(g, settings, bad):
    with pytest.raises(g.ArgumentError) as e:
        g.gDCA_multi(SMALL, settings)
    # exactly the message check_arguments (and so gDCA) gives for the offending setting
    with pytest.raises(g.ArgumentError) as e1:
        g.check_arguments(SMALL, bad[0], ":auto", 0.9, bad[1], 5)
    assert str(e.value) == str(e1.value) and str(e.value).startswith(("invalid pseudocount value", "invalid score value"))


def test_other_arguments_and_the_shape_of_settings(g, tmp_path):
    for kw, msg in [(dict(theta=1.5), "invalid θ value"), (dict(θ=":bogus"), "invalid θ value"),
                    (dict(max_gap_fraction=2.0), "invalid max_gap_fraction value"), (dict(min_separation=0), "invalid min_separation value")]:
        with pytest.raises(g.ArgumentError, match=re.escape(msg)):
            g.gDCA_multi(SMALL, [(0.8, "frob")], **kw)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_multi(str(tmp_path / "missing.fasta"), [(0.8, "frob")])
    for settings in ([], [(0.8, "frob")] * 17):
        with pytest.raises(g.ArgumentError, match="invalid number of settings"):
            g.gDCA_multi(SMALL, settings)
    for settings in ([0.8], [(0.8,)], 5):
        with pytest.raises(g.ArgumentError):
            g.gDCA_multi(SMALL, settings)
    with pytest.raises(TypeError):
        g.gDCA_multi(SMALL, [(0.8, "frob")], pseudocount=0.8)
    assert g.gDCA_multi is g.gdca.gDCA_multi and "gDCA_multi" not in g.__all__


def test_without_a_device_it_raises(g):
    if g.load().gdca_device_count() > 0:
        pytest.skip("a HIP device is visible here")
    with pytest.raises(g.GdcaError):
        g.gDCA_multi(SMALL, [(0.8, ":frob"), (0.2, ":DI")])
    assert g.gdca.last_multi_stats is None


def test_cov_from_pij_is_listed_without_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None:
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--sources", "k_tally.hip", "--kernels", "none"],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if "k_cov_from_pij" in ln]
    assert len(rows) == 2, r.stdout                      # the launch of its own and the batched form
    for row in rows:
        vgpr, agpr, vsp, ssp, scratch = (int(x) for x in row[-7:-2])
        assert vsp == 0 and ssp == 0 and scratch == 0, row
    assert all(int(row[-2]) >= 1 for row in rows)        # occupancy reported
