#!/usr/bin/env python3
"""Device time of the pair log-odds (gdca_run_pair_logodds_dev) at the two shapes of DESIGN 3.7, and that nothing existing pays for it:

  (1) the cost of the score: gdca_run_pair_logodds of this library against gdca_run_pair_energies (ENERGY) of the PARENT commit's
      library (--parent-lib: a libgdca.so built from the parent), alternating inside this one process A B B A; the marginal fits'
      share (info ms_marginals) beside (n_A^3 + n_B^3) / n^3, their share of the joint sweep's flops;
  (2) gdca_run_pair_energies (both `what`) and gdca_run_partner_match of this library against the parent's, A B B A: the new medians
      are expected inside the parent's min .. max;
  (3) --use: on the recorded family of tests/logodds_model.py, the natives recovered by the assignment on L, on E and on R.

One process; contexts are made before anything is timed; HIP events on the stream the contexts work on (so the host round trips of
the three collects of a log-odds run are inside its time), 10 timed repeats after 2 per block, medians over a side's two blocks; every
GPU step under a time limit of its own (a step that overruns ends the process with status 124, nothing is started after it), and
the process exits on the first failure.

    python tools/logodds_bench.py --config B --parent-lib PATH --out profiles/logodds_bench.json   (N = 128, split = 64, M = 10 000, K = 4096)
    python tools/logodds_bench.py --config C --parent-lib PATH --out profiles/logodds_bench.json   (N = 500, split = 250, M = 50 000, K = 8192)
Results of several configs are merged into one JSON file by config name."""
import argparse
import contextlib
import ctypes as C
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")

CONFIGS = {"B": dict(N=128, split=64, M=10000, K=4096, theta=0.2, seed=0xB128),
           "C": dict(N=500, split=250, M=50000, K=8192, theta=-1.0, seed=0xC500)}


@contextlib.contextmanager
def step_limit(seconds, what):
    def over():
        sys.stderr.write("logodds_bench: step '%s' exceeded %d s\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    t = threading.Timer(seconds, over)
    t.daemon = True
    t.start()
    try:
        yield
    finally:
        t.cancel()


def timed(fn, warmup, repeats):
    """HIP events on the current torch stream (the contexts were made on it) -> list of ms"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def parent_context(gd, path, stream):
    """A Context on another build of the library: the binding's prototypes on the symbols that build has"""
    lib = C.CDLL(path)
    for name, (res, args) in gd._lib.SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:  # (a symbol newer than the parent)
            continue
        fn.restype, fn.argtypes = res, args
    ctx = object.__new__(gd.Context)
    ctx.lib, h = lib, C.c_void_p()
    if lib.gdca_ctx_create_on_stream(0, C.c_void_p(stream), C.byref(h)) != 0:
        sys.exit("logodds_bench: no context on the parent's library")
    ctx.h, ctx.device = h, 0
    return ctx


def abba(run_parent, run_new, warmup, repeats):
    """A B B A -> (parent samples, new samples)"""
    p1 = timed(run_parent, warmup, repeats)
    n1 = timed(run_new, warmup, repeats)
    n2 = timed(run_new, warmup, repeats)
    p2 = timed(run_parent, warmup, repeats)
    return p1 + p2, n1 + n2


def summary(parent, new):
    return dict(parent_median=statistics.median(parent), parent_min=min(parent), parent_max=max(parent), new_median=statistics.median(new),
                new_min=min(new), new_max=max(new), ratio=statistics.median(new) / statistics.median(parent),
                new_median_inside_parent_spread=bool(min(parent) <= statistics.median(new) <= max(parent)), parent_all=parent, new_all=new)


def the_use(gd):
    """natives recovered by the assignment on L, on E and on R on the recorded family (tests/logodds_model.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import logodds_model as lo

    Zfit, Zheld = lo.family_alignment()
    Zheld = Zheld[np.random.default_rng(lo.SPECIES_SEED).permutation(Zheld.shape[0])]
    f = lo.FAMILY
    split, q = f["split"], f["q"]
    XA, XB = np.asfortranarray(Zheld[:, :split].T), np.asfortranarray(Zheld[:, split:].T)
    Zf = np.asfortranarray(Zfit.T)
    N, M = Zf.shape
    off = np.concatenate(([0], np.cumsum(lo.SPECIES_SIZES))).astype(np.int32)
    K = XA.shape[1]
    ctx = gd.Context(0)
    out = {}
    (_, match, _, info), _ = ctx.run_partner_logodds_ptr(Zf.ctypes.data, N, M, q, f["pseudocount"], -1.0, split, XA.ctypes.data, K, XB.ctypes.data, K, off,
                                                        off, want_blocks=False)
    out["natives_L"] = int(np.sum(match == np.arange(K)))
    out["information"] = info["information"]
    for what, key in ((gd._lib.PAIR_ENERGY, "natives_E"), (gd._lib.PAIR_COUPLING, "natives_R")):
        (_, match, _), _ = ctx.run_partner_match_ptr(Zf.ctypes.data, N, M, q, f["pseudocount"], -1.0, split, XA.ctypes.data, K, XB.ctypes.data, K, off, off,
                                                     what, want_blocks=False)
        out[key] = int(np.sum(match == np.arange(K)))
    (L, _, _, _), _ = ctx.run_pair_logodds_ptr(Zf.ctypes.data, N, M, q, f["pseudocount"], -1.0, split, XA.ctypes.data, K, XB.ctypes.data, K)
    E, _ = ctx.run_pair_energies_ptr(Zf.ctypes.data, N, M, q, f["pseudocount"], -1.0, split, XA.ctypes.data, K, XB.ctypes.data, K)
    out["row_best_native_L"] = float((L.argmax(axis=1) == np.arange(K)).mean())
    out["row_best_native_E"] = float((E.argmin(axis=1) == np.arange(K)).mean())
    out["pairs"], out["species_sizes"] = K, list(lo.SPECIES_SIZES)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B", choices=sorted(CONFIGS))
    ap.add_argument("--parent-lib", required=True, help="libgdca.so built from the parent commit")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--use", action="store_true", help="also the natives recovered on the recorded family")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logodds_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, split, M, K, q, theta, pc = c["N"], c["split"], c["M"], c["K"], 21, c["theta"], args.pseudocount
    s = q - 1
    n, nA, nB = N * s, split * s, (N - split) * s
    ENERGY, COUPLING = gd._lib.PAIR_ENERGY, gd._lib.PAIR_COUPLING
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from partner_bench import species_sizes

    sizes = species_sizes(K)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    pairings = int(sum(k * k for k in sizes))
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        new = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        old = parent_context(gd, args.parent_lib, stream.cuda_stream)
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dXA = dZ[:K, :split].contiguous()   # column-major split x K
        dXB = dZ[:K, split:].contiguous()
        dE = torch.empty(K * K, dtype=torch.float64, device="cuda")
        dE2 = torch.empty(K * K, dtype=torch.float64, device="cuda")
        dEb = torch.empty(pairings, dtype=torch.float64, device="cuda")
        dmatch = torch.empty(K, dtype=torch.int32, device="cuda")
        dgap = torch.empty(K, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, split=split, M=M, KA=K, KB=K, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats,
               warmup=args.warmup, flop_ratio_marginals=(float(nA) ** 3 + float(nB) ** 3) / float(n) ** 3)
    Z, XA, XB = dZ.data_ptr(), dXA.data_ptr(), dXB.data_ptr()
    last = {}

    def pair(ctx, what, out):
        return lambda: ctx.run_pair_energies_dev(Z, N, M, q, pc, theta, split, XA, K, XB, K, what, out.data_ptr())

    def logodds():
        last["info"], last["st"] = new.run_pair_logodds_dev(Z, N, M, q, pc, theta, split, XA, K, XB, K, dE2.data_ptr())

    def partner(ctx):
        return lambda: ctx.run_partner_match_dev(Z, N, M, q, pc, theta, split, XA, K, XB, K, off, off, ENERGY, dEb.data_ptr(), dmatch.data_ptr(),
                                                 dgap.data_ptr())

    with step_limit(600, "(1) the log-odds against the parent's pair energies"):
        res["logodds_vs_parent_pair_energies"] = summary(*abba(pair(old, ENERGY, dE), logodds, args.warmup, args.repeats))
        info, st = last["info"], last["st"]
        res["ms_marginals"], res["ms_total_stats"], res["ms_inverse_joint"] = info["ms_marginals"], st["ms_total"], st["ms_inverse"]
        res["ms_score"], res["ms_pair_tally"], res["ms_covariance"] = st["ms_score"], st["ms_pair_tally"], st["ms_covariance"]
        res["marginals_share_of_total"] = info["ms_marginals"] / st["ms_total"]
        res["marginals_over_joint_inverse"] = info["ms_marginals"] / st["ms_inverse"]
        res["information"] = info["information"]
        # the score is the expression of its parts: E of the parent's library on the same fit, bit for bit
        old.run_pair_energies_dev(Z, N, M, q, pc, theta, split, XA, K, XB, K, ENERGY, dE.data_ptr())
        dA, dB = torch.empty(K, dtype=torch.float64, device="cuda"), torch.empty(K, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        info, _ = new.run_pair_logodds_dev(Z, N, M, q, pc, theta, split, XA, K, XB, K, dE2.data_ptr(), dA.data_ptr(), dB.data_ptr())
        want = ((dA[None, :] + dB[:, None]) - dE.view(K, K)) + info["information"]   # (row-major view: [b, a])
        res["L_is_the_expression_of_the_parents_E"] = bool(torch.equal(want, dE2.view(K, K)))
    with step_limit(600, "(2) nothing existing pays"):
        res["pair_energy"] = summary(*abba(pair(old, ENERGY, dE), pair(new, ENERGY, dE2), args.warmup, args.repeats))
        res["pair_energy_bits_equal"] = bool(torch.equal(dE, dE2))
        res["pair_coupling"] = summary(*abba(pair(old, COUPLING, dE), pair(new, COUPLING, dE2), args.warmup, args.repeats))
        res["pair_coupling_bits_equal"] = bool(torch.equal(dE, dE2))
        res["partner_match"] = summary(*abba(partner(old), partner(new), args.warmup, args.repeats))
    old.lib.gdca_ctx_destroy(old.h)
    old.h = None
    new.close()
    if args.use:
        with step_limit(120, "(3) the use"):
            res["use"] = the_use(gd)

    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[args.config] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(allres, f, indent=1, sort_keys=True)
        f.write("\n")

    def brief(v):
        return {k: x for k, x in v.items() if not k.endswith("_all")} if isinstance(v, dict) else v

    print(json.dumps({k: brief(v) for k, v in res.items()}, sort_keys=True))
    ok = res["L_is_the_expression_of_the_parents_E"] and res["pair_energy_bits_equal"] and res["pair_coupling_bits_equal"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
