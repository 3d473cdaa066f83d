"""The greedy walk stated in numpy (the checker of tests/test_walk_cpu.py and tests/test_gpu_walk.py).  Conventions of
tests/mutation_model.py (s = q - 1, r(i, c) = i s + c - 1, the gap q has no row, V(x; i, q) = +0.0) and the rule of include/gdca.h,
"greedy walk":

    dE(i, b) = V[i][b] - V[i][x_i]                              one f64 subtraction of two table entries
    the step: the admissible (i, b) that minimises dE, ties to the smallest code i q + (b - 1), a NaN never; taken if dE < -min_gain
    V[j][c] = V[j][c] + (K(j,c; i,b) - K(j,c; i,a))             j != i, c in 1..s: one subtraction, then one addition;
                                                                K(j,c; i,b) = mJ[r(j,c), r(i,b)], +0.0 where b is the gap

  emulate        (a) the rule in float64, operation for operation, from a GIVEN initial table; reads the library's lower triangle of mJ only
                 (sym_column);
  replay_exact   (b) the exact potentials (mutation_model.potentials_exact, np.longdouble) of every state a recorded path visits;
  walk_bounds    (c) what (a) or the device may differ from (b) by.

THE BOUNDS (u = 2^-53, everything per table entry [j][c], c a residue; the gap column is exact).  Write V*_t for the exact potentials
of the state x_t, e_t for a bound on |V_t - V*_t| of the walked table, dk_t = K_b - K_a of step t (the step from x_t to x_t+1).
  the start   V_0 is a mutation scan of x_0 (any summation order): e_0 = bound_V(B_0) of tests/mutation_model.py.
  a step      V_t+1 = fl(V_t + fl(dk_t)) while V*_t+1 = V*_t + dk_t exactly (the potentials of x_t+1 differ from those of x_t by the two
              columns; the moved site's own row does not depend on its symbol and is not touched: e_t+1 = e_t there).
              |fl(dk) - dk| <= u |dk|, and the addition's error is at most u times its exact result, whose size is at most
              |V*_t+1| + e_t + u |dk|.  Together
                  e_t+1 <= (e_t + u (|dk_t| + |V*_t+1|)) (1 + u),
              so the table after T steps is within bound_V(B_0) + sum over t <= T of u (|K_b - K_a| + |V_t|) (1 + O(u)) of the exact
              potentials of x_T.  The recurrence below carries the factor 1 + u explicitly.
  a dE        the recorded dE_t = fl(V_t[i][b] - V_t[i][a]) against dE*_t = V*_t[i][b] - V*_t[i][a]:
                  |dE_t - dE*_t| <= e_t[i][b] + e_t[i][a] + 2 u |dE*_t|
              (the two entries and the one subtraction; the 2 as in mutation_model.delta_bound).  The issue that set this checker's
              terms states the same bound as delta_bound AT THE STATE x_t (its B_t in the place of B_0) plus the drift of the two
              entries; the two differ in which state's absolute sums carry the scan's part.  walk_bounds returns the SMALLER of the
              two per entry, so a result that passes satisfies both.
No tolerance is invented in a test: they all come from here, from mutation_model.py and from energy_model.py."""
import numpy as np

import mutation_model as mm
from energy_model import U

GAP_TARGET, FILL_GAPS = 1, 2


def sym_column(mJ, r):
    """column r of the symmetric matrix from the triangle the LIBRARY reads alone.  The library takes the matrix column-major and reads
    element (row, col), row >= col, at [col * n + row]; the Python wrappers hand it the row-major array as it lies, so that element is
    mJ[col, row] here -- numpy's upper triangle: rows r' >= r of the column as mJ[r, r'], rows r' < r mirrored, mJ[r', r]"""
    return np.concatenate((mJ[:r, r], mJ[r, r:]))


def admissible(x, q, mask, flags):
    """(N, q) bool: the moves (i, b) the rule admits in state x (symbols 1..q)"""
    N = x.shape[0]
    a = np.asarray(x, dtype=np.int64) - 1
    adm = np.ones((N, q), dtype=bool)
    adm[np.arange(N), a] = False
    if mask is not None:
        adm &= (np.asarray(mask) != 0)[:, None]
    if not flags & FILL_GAPS:
        adm &= (a != q - 1)[:, None]
    if not flags & GAP_TARGET:
        adm[:, q - 1] = False
    return adm


def emulate(V0, mJ, x, q, mask=None, flags=0, min_gain=0.0, max_steps=1):
    """(a) -> (xout (N,) int8, steps, path (max_steps, 2) int32, dE_path (max_steps,), dE_sum, V (N, q)): what the library returns for one
    sequence x (N symbols 1..q) whose initial table is V0 (N, q) -- bit for bit, if the library follows the rule"""
    x = np.array(x, dtype=np.int64)
    N, s = x.shape[0], q - 1
    V = np.array(V0, dtype=np.float64)
    assert V.shape == (N, q)
    path = np.full((max_steps, 2), -1, dtype=np.int32)
    dE_path = np.zeros(max_steps)
    steps, total = 0, 0.0
    sites = np.arange(N)
    zero = np.zeros(N * s)  # (+0.0: the gap's column)
    while steps < max_steps:
        a = x - 1
        with np.errstate(invalid="ignore"):
            dE = V - V[sites, a][:, None]
        ok = admissible(x, q, mask, flags) & ~np.isnan(dE)
        if not ok.any():
            break
        code = int(np.argmin(np.where(ok, dE, np.inf)))  # (the first entry that reaches the minimum: the smallest code; -0.0 == +0.0)
        i, b = divmod(code, q)
        best = dE[i, b]
        if not ok[i, b] or not best < -min_gain:  # (only +inf admissible entries: argmin may name an inadmissible one)
            break
        path[steps] = (i, b + 1)
        dE_path[steps] = best
        total = total + best
        steps += 1
        kb = sym_column(mJ, i * s + b) if b < s else zero
        ka = sym_column(mJ, i * s + a[i]) if a[i] < s else zero
        dk = (kb - ka).reshape(N, s)
        keep = V[i].copy()
        V[:, :s] = V[:, :s] + dk
        V[i] = keep
        x[i] = b + 1
    return x.astype(np.int8), steps, path, dE_path, total, V


def states_of(x0, path, steps):
    """(N, steps + 1) int8: the states x_0 .. x_steps a path visits"""
    X = np.repeat(np.asarray(x0, dtype=np.int8)[:, None], steps + 1, axis=1)
    for t in range(steps):
        X[path[t, 0], t + 1:] = path[t, 1]
    return np.asfortranarray(X)


def replay_exact(mJ, Pi, x0, path, q, steps=None):
    """(b) -> (X (N, T + 1) the visited states, Vl (T + 1, N, q) longdouble exact potentials, B (T + 1, N, q) their absolute-value sums,
    dEl (T + 1, N, q) longdouble: the exact dE of EVERY move in every state)"""
    path = np.asarray(path)
    T = int((path[:, 0] >= 0).sum()) if steps is None else int(steps)
    X = states_of(x0, path, T)
    _, B, Vl = mm.potentials_exact(mJ, Pi, X, q)
    dEl = Vl - mm.wild_type(Vl, X, q)
    return X, Vl, B, dEl


def walk_bounds(mJ, X, path, q, Vl, B, dEl):
    """(c) -> (e (T + 1, N, q): the bound on |table - exact potentials| in every state, bD (T + 1, N, q): the bound on |dE - exact dE|
    of every move in every state).  X, Vl, B, dEl: replay_exact's."""
    N, T1 = X.shape
    s = q - 1
    absV = np.abs(Vl).astype(np.float64) * (1 + U)
    absD = np.abs(dEl).astype(np.float64) * (1 + U)
    e = np.zeros((T1, N, q))
    e[0] = mm.bound_V(N, q, B[0])
    drift = np.zeros((T1, N, q))  # e_t - e_0: what the steps alone add
    zero = np.zeros(N * s, dtype=np.longdouble)
    for t in range(T1 - 1):
        i, b = int(path[t, 0]), int(path[t, 1]) - 1
        a = int(X[i, t]) - 1
        kb = sym_column(mJ, i * s + b).astype(np.longdouble) if b < s else zero
        ka = sym_column(mJ, i * s + a).astype(np.longdouble) if a < s else zero
        adk = (np.abs(kb - ka).astype(np.float64) * (1 + U)).reshape(N, s)
        nxt = e[t].copy()
        nxt[:, :s] = (e[t][:, :s] + U * (adk + absV[t + 1][:, :s])) * (1 + U)
        nxt[i] = e[t][i]
        e[t + 1] = nxt
        drift[t + 1] = nxt - e[0]
    own = lambda A, t: A[np.arange(N), X[:, t].astype(np.int64) - 1][:, None]  # noqa: E731  (N, 1): the entry of each site's own symbol in state t
    bD = np.empty((T1, N, q))
    for t in range(T1):
        mine = e[t] + own(e[t], t) + 2.0 * U * absD[t]
        bv = mm.bound_V(N, q, B[t])
        stated = bv + own(bv, t) + 2.0 * U * absD[t] + drift[t] + own(drift[t], t)
        bD[t] = np.minimum(mine, stated)
    return e, bD


def check_walk(mJ, Pi, x0, q, mask, flags, min_gain, max_steps, steps, path, dE_path, V_final, tag=""):
    """One walk's outputs (the library's or emulate's) against (b) within (c): every recorded dE, the final table, every chosen move
    against the exact minimum of its state, and -- a walk that stopped before max_steps -- the local minimum.  Returns
    (sum of the steps' dE bounds, the largest error / bound seen)."""
    X, Vl, B, dEl = replay_exact(mJ, Pi, x0, path, q, steps)
    e, bD = walk_bounds(mJ, X, path, q, Vl, B, dEl)
    worst, total = 0.0, 0.0
    for t in range(steps):
        i, b = int(path[t, 0]), int(path[t, 1]) - 1
        adm = admissible(X[:, t], q, mask, flags)
        assert adm[i, b], (tag, t, i, b)
        err = abs(float(np.longdouble(dE_path[t]) - dEl[t, i, b]))
        assert err <= bD[t, i, b], (tag, t, err, bD[t, i, b])
        worst = max(worst, err / bD[t, i, b])
        total += bD[t, i, b]
        # the chosen move against the exact minimiser m: exact(c) <= exact(m) + bound(c) + bound(m) <= exact(m) + twice the larger
        ex = np.where(adm, dEl[t].astype(np.float64), np.inf)
        m = np.unravel_index(int(np.argmin(ex)), ex.shape)
        assert float(dEl[t, i, b] - dEl[t][m]) <= bD[t, i, b] + bD[t][m], (tag, t, "not the minimum")
        assert dE_path[t] < -min_gain
    errV = np.abs((np.asarray(V_final).astype(np.longdouble) - Vl[steps]).astype(np.float64))
    assert np.all(errV <= e[steps]), (tag, float((errV[:, :q - 1] / e[steps][:, :q - 1]).max()))
    assert np.all(np.asarray(V_final)[:, q - 1] == 0.0) and not np.signbit(np.asarray(V_final)[:, q - 1]).any()
    worst = max(worst, float((errV[:, :q - 1] / e[steps][:, :q - 1]).max()))
    if steps < max_steps:  # stopped by itself: a local minimum up to the bound
        adm = admissible(X[:, steps], q, mask, flags)
        ex = dEl[steps].astype(np.float64)
        assert np.all(ex[adm] >= -min_gain - bD[steps][adm]), (tag, "not a local minimum")
    return total, worst
