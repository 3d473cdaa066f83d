"""The schedule of the persistent SPD-inverse sweep (csrc/gdca_sweep_schedule.h), on the CPU: the header is plain C++
shared by k_inverse.hip (plan_sweep on the host, the decode in the kernels) and this test, which compiles it alone with the host
compiler and calls it through ctypes.

1. Every field of the schedule equals the rules as they stood before the header existed, restated below in Python from plan_sweep.
2. The two lists cover the work exactly once: an enumerator (C++, flat arrays) walks main_decode over the whole main list and
   chain_decode over the whole M list and counts, group by group, what they name -- update tiles, write-backs, panel halves, M items --
   against what the sweep needs, and where rem_tail puts the tail of a group's remainder tiles; the flag block's regions do not
   overlap and fit what the workspace sets aside."""
import ctypes
import os
import shutil
import subprocess

import pytest

from gdca_testutil import _SCHEDULES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussdca.jl_amd", "csrc")
T, SLAB_ITEMS = 128, 8
CUS = 256

ENUMERATOR = r'''
#include <stdio.h>
#include <string.h>
#include <vector>
#include "gdca_sweep_schedule.h"
using namespace gdca_sweep;

static_assert(GDCA_SWEEP_TILE == 128 && GDCA_SWEEP_KC == 16 && GDCA_SWEEP_SLAB_ITEMS == 8 && GDCA_SWEEP_MAX_MERGE == 8, "");

static Tuning tuning_of(const int *tu, long timeout_ms)
{
    return Tuning{tu[0], tu[1], tu[2], tu[3], tu[4], tu[5], tu[6], tu[7], tu[8], tu[9], tu[10], timeout_ms};
}

// the schedule's scalars: ints[18], ticks[2], chunks; the three tables stay in `table` (item0 | mitem0 | gs, ng + 1 entries each)
extern "C" void schedule(int nblk, int n_real, int cus, const int *tu, long timeout_ms, int merged, int members, int *table, int *ints,
                         unsigned long long *ticks, double *chunks)
{
    const Schedule S = sweep_schedule(nblk, n_real, cus, tuning_of(tu, timeout_ms), merged != 0, members, table);
    const int v[18] = {S.nblk, S.g, S.ng, S.total, S.total_m, S.pro, S.rem_tail, S.ppb, S.n_mcu, S.mcu_solo, S.ring, S.slab, S.n_real, S.rl,
                       S.table_ints, (int)(S.item0 - table), (int)(S.mitem0 - table), (int)(S.gs - table)};
    memcpy(ints, v, sizeof(v));
    ticks[0] = S.timeout_ticks;
    ticks[1] = S.hole_timeout_ticks;
    *chunks = S.chunks;
}

extern "C" int chunks_of_group(int nblk, int n_real, int cus, const int *tu, int merged, int *table, int p)
{
    const Schedule S = sweep_schedule(nblk, n_real, cus, tuning_of(tu, 0), merged != 0, 1, table);
    return g_chunks(S, p);
}

extern "C" void flags(int nblk, int ng, unsigned long long *out)
{
    const FlagLayout L = flag_layout(nblk, ng);
    const size_t v[12] = {L.gen, L.rb, L.mc, L.done, L.sl, L.next, L.next_m, L.mxcc, L.arrived, L.mcu, L.abort, L.words};
    for (int k = 0; k < 12; ++k) out[k] = v[k];
    out[12] = flag_words_max(nblk);
    out[13] = (unsigned long long)table_ints_max(nblk);
}

// ---- the lists cover the work exactly once ------------------------------------------------------------------------------------------
struct Count {
    const Schedule &S;
    int nblk, ng, ntri;
    std::vector<unsigned char> tile;   // [ng][ntri]: times tile (I, J), J <= I, of update p was named
    std::vector<unsigned char> wb;     // [ng][nblk * 4]: times write-back item e of group p was named
    std::vector<unsigned char> half;   // [ng][nblk]: the panel halves of group p row block i has received, one bit a half (2 sz of them)
    std::vector<unsigned char> m;      // [ng][128]: times M item e of group p was named
    std::vector<int> slab;             // [ng][3]: slab, xslab, slab2 items of group p named
    std::vector<long long> done;       // [ng]: tiles and write-backs named
    long long bad = 0;
    char *msg;
    int msglen;
    Count(const Schedule &S_, char *msg_, int msglen_)
        : S(S_), nblk(S_.nblk), ng(S_.ng), ntri(S_.nblk * (S_.nblk + 1) / 2), tile((size_t)ng * ntri), wb((size_t)ng * nblk * 4), half((size_t)ng * nblk),
          m((size_t)ng * 128), slab((size_t)ng * 3), done(ng), msg(msg_), msglen(msglen_)
    {
    }
    void fail(const char *what, int p, int a, int b)
    {
        if (bad++ == 0) snprintf(msg, msglen, "%s: group %d, (%d, %d)", what, p, a, b);
    }
    bool group_ok(int p, const char *what)
    {
        if (p >= 0 && p < ng) return true;
        fail(what, p, -1, -1);
        return false;
    }
    bool in_group(int p, int i) const { return i >= S.gs[p] && i < S.gs[p + 1]; }
    static void bump(unsigned char &c)
    {
        if (c < 255) ++c;
    }
    void name_tile(int p, int I, int J, const char *src)
    {
        if (!group_ok(p, src)) return;
        if (J < 0 || J > I || I >= nblk) return fail("tile out of the lower triangle", p, I, J);
        if (in_group(p, I) || in_group(p, J)) return fail("tile with an index in its own group", p, I, J);
        bump(tile[(size_t)p * ntri + (size_t)I * (I + 1) / 2 + J]);
        ++done[p];
    }
    void name_wb(int p, int e)
    {
        if (!group_ok(p, "write-back")) return;
        const int sz = S.gs[p + 1] - S.gs[p];
        if (e < 0 || e >= (nblk - sz) * sz) return fail("write-back index out of range", p, e, 0);
        bump(wb[(size_t)p * nblk * 4 + e]);
        ++done[p];
    }
    // halves h0 .. h0 + n - 1 of group p's panel of row block i
    void name_halves(int p, int i, int h0, int n, const char *src)
    {
        if (!group_ok(p, src)) return;
        const int sz = S.gs[p + 1] - S.gs[p];
        if (i < 0 || i >= nblk || in_group(p, i)) return fail("panel of a row block inside its group, or of none", p, i, h0);
        if (h0 < 0 || h0 + n > 2 * sz) return fail("panel part out of range", p, i, h0);
        for (int h = h0; h < h0 + n; ++h) {
            if (half[(size_t)p * nblk + i] & (1u << h)) fail("panel half named twice", p, i, h);
            half[(size_t)p * nblk + i] |= (unsigned char)(1u << h);
        }
    }
};

// returns the number of violations (the first one described in msg); 0 = the lists of this schedule cover the work exactly once
extern "C" long long coverage(int nblk, int n_real, int cus, const int *tu, int merged, int members, char *msg, int msglen)
{
    std::vector<int> table((size_t)table_ints_max(nblk));
    const Schedule S = sweep_schedule(nblk, n_real, cus, tuning_of(tu, 0), merged != 0, members, table.data());
    Count C(S, msg, msglen);
    msg[0] = 0;
    const int ng = S.ng;
    if (S.table_ints > table_ints_max(nblk)) C.fail("item table larger than its room", -1, S.table_ints, table_ints_max(nblk));
    // the main list
    int p = 0;
    // (the order inside a group's sequence, as far as rem_tail sets it: behind its last panel item come the last min(rem_tail, n_rem)
    // remainder slots and nothing else -- and in front of those, where the last row of panel(p+1) is the chain's, that row's empty slots)
    int after = -1;  // items of the running group's sequence behind its last panel item (-1: no panel item yet)
    auto tail_ok = [&](int g) {
        if (after < 0) return;
        const int sz = S.gs[g + 1] - S.gs[g], nsz = g + 1 < ng ? S.gs[g + 2] - S.gs[g + 1] : 0, nrest = nblk - sz - nsz;
        const int nrem = nrest > 0 ? nrest * (nrest + 1) / 2 : 0;
        const int chain_row_last = S.slab && S.gs[g + 1] + 3 == nblk ? S.ppb * nsz : 0;
        if (after != (nrem < S.rem_tail ? nrem : S.rem_tail) + chain_row_last) C.fail("remainder slots behind the last panel item against rem_tail", g, after, S.rem_tail);
    };
    for (int item = 0; item < S.total; ++item) {
        const int before = p;
        const MainItem it = main_decode(S, p, item);
        if (p < before || p >= ng) {
            C.fail("running group of the main list", p, item, before);
            break;
        }
        if (p != before) {
            tail_ok(before);
            after = -1;
        }
        if (item >= S.pro) {
            if (it.kind == 0)
                after = 0;
            else if (after >= 0) {
                ++after;
                if (it.kind != 1 && it.kind != 3) C.fail("behind the panel items of a sequence: not a remainder slot", p, item, it.kind);
            }
        }
        if (it.kind == 1 || it.kind == 4) {
            if (it.p != p) C.fail("tile item of another group than the running one", it.p, it.a, it.b);
            C.name_tile(it.p, it.a, it.b, "main-list tile");
        } else if (it.kind == 2) {
            if (it.p != p) C.fail("write-back item of another group than the running one", it.p, it.a, it.b);
            C.name_wb(it.p, it.a);
        } else if (it.kind == 0) {
            // part b of ppb sz parts: one half (ppb = 2) or a 128 x 128 item, two halves (ppb = 1)
            C.name_halves(it.p, it.a, it.b * (2 / S.ppb), 2 / S.ppb, "main-list panel");
        } else if (it.kind != 3)
            C.fail("main-list item of an unknown kind", p, item, it.kind);
    }
    if (ng > 0) tail_ok(p);
    // the M list
    int q = 0;
    for (int item = 0; item < S.total_m; ++item) {
        const int before = q;
        const ChainItem it = chain_decode(S, q, item);
        if (q < before || q >= ng || it.q != q) {
            C.fail("running group of the M list", q, item, before);
            break;
        }
        const int b0 = S.gs[q], sz = S.gs[q + 1] - b0;
        if (it.kind == CHAIN_M) {
            if (it.a < 0 || it.a >= m_items(sz))
                C.fail("M item out of range", q, it.a, 0);
            else
                Count::bump(C.m[(size_t)q * 128 + it.a]);
        } else if (it.kind == CHAIN_SLAB || it.kind == CHAIN_XSLAB || it.kind == CHAIN_SLAB2) {
            if (!S.slab || it.a < 0 || it.a >= GDCA_SWEEP_SLAB_ITEMS) C.fail("slab item out of range, or outside a slab schedule", q, it.kind, it.a);
            ++C.slab[(size_t)q * 3 + (it.kind - CHAIN_SLAB)];
        } else if (it.kind == CHAIN_MPANEL) {
            if (q + 1 >= ng || it.a < S.gs[q + 1] || it.a >= S.gs[q + 2]) C.fail("chain panel item outside the next group's rows", q, it.a, it.b);
            C.name_halves(q, it.a, it.b, 1, "chain panel");
        } else if (it.kind == CHAIN_DIAG) {
            C.name_tile(q, it.a, it.b, "chain tile");
        } else
            C.fail("M-list item of an unknown kind", q, item, it.kind);
    }
    // the slab items: SLAB_ITEMS of a kind together are one tile (and, slab and slab2, the two halves of a row's panel)
    for (int g = 0; g < ng; ++g) {
        const int b0 = S.gs[g];
        for (int k = 0; k < 3; ++k) {
            const int n = C.slab[(size_t)g * 3 + k];
            if (n == 0) continue;
            if (n != GDCA_SWEEP_SLAB_ITEMS) {
                C.fail("not one set of slab items", g, k, n);
                continue;
            }
            if (k == 0) {
                C.name_tile(g, b0 + 1, b0 + 1, "slab");
                C.name_halves(g, b0 + 1, 0, 2, "slab");
            } else if (k == 1)
                C.name_tile(g, b0 + 2, b0 + 1, "xslab");
            else {
                C.name_tile(g, b0 + 2, b0 + 2, "slab2");
                C.name_halves(g, b0 + 2, 0, 2, "slab2");
            }
        }
    }
    // every group: each tile, write-back, panel half and M item exactly once
    for (int g = 0; g < ng; ++g) {
        const int b0 = S.gs[g], c0 = S.gs[g + 1], sz = c0 - b0, pn = nblk - sz;
        if (sz < 1 || sz > 4) C.fail("group size", g, sz, 0);
        for (int I = 0; I < nblk; ++I)
            for (int J = 0; J <= I; ++J) {
                const bool inside = C.in_group(g, I) || C.in_group(g, J);
                const int n = C.tile[(size_t)g * C.ntri + (size_t)I * (I + 1) / 2 + J];
                if (n != (inside ? 0 : 1)) C.fail(n ? "tile named more than once" : "tile never named", g, I, J);
            }
        for (int e = 0; e < pn * sz; ++e)
            if (C.wb[(size_t)g * nblk * 4 + e] != 1) C.fail("write-back not named exactly once", g, e, C.wb[(size_t)g * nblk * 4 + e]);
        if (C.done[g] != (long long)g_done_total(S, g)) C.fail("tiles plus write-backs against g_done_total", g, (int)C.done[g], (int)g_done_total(S, g));
        for (int i = 0; i < nblk; ++i) {
            const unsigned want = C.in_group(g, i) ? 0u : (1u << (2 * sz)) - 1u;
            if (C.half[(size_t)g * nblk + i] != want) C.fail("panel halves of a row block", g, i, C.half[(size_t)g * nblk + i]);
        }
        for (int e = 0; e < 128; ++e)
            if (C.m[(size_t)g * 128 + e] != (e < m_items(sz) ? 1 : 0)) C.fail("M item not named exactly once", g, e, C.m[(size_t)g * 128 + e]);
    }
    if (ng > 0 && S.gs[ng] != nblk) C.fail("groups do not end at the last block", ng, S.gs[ng], nblk);
    return C.bad;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    d = tmp_path_factory.mktemp("schedule")
    # the header alone, as the issue of this test states it
    alone = d / "alone.cpp"
    alone.write_text('#include "gdca_sweep_schedule.h"\n')
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(alone)], check=True)
    src = d / "enumerator.cpp"
    src.write_text(ENUMERATOR)
    so = d / "enumerator.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)],
                   check=True)
    lib = ctypes.CDLL(str(so))
    ip = ctypes.POINTER(ctypes.c_int)
    lib.schedule.restype = None
    lib.schedule.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ctypes.c_long, ctypes.c_int, ctypes.c_int, ip, ip,
                             ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_double)]
    lib.chunks_of_group.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ctypes.c_int, ip, ctypes.c_int]
    lib.flags.restype = None
    lib.flags.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong)]
    lib.coverage.restype = ctypes.c_longlong
    lib.coverage.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    return lib


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
# gdca_tuning's defaults (gdca_tuning_from_env) of the switches the schedule reads, in the order of gdca_sweep::Tuning
FIELDS = ("group", "ramp", "ragged", "rem_tail", "panel_halves", "slab", "ring", "mcus", "mcu_solo", "merge_group", "merge_mcus")
DEFAULTS = dict(group=-1, ramp=1, ragged=1, rem_tail=-1, panel_halves=-1, slab=1, ring=8, mcus=-1, mcu_solo=-1, merge_group=-1, merge_mcus=-1)
NBLKS = tuple(range(1, 81)) + (94, 128, 157)
MEMBERS = 8  # a merged launch's


def tuning(**kv):
    t = dict(DEFAULTS)
    t.update(kv)
    return t


def settings():
    """(tuning, merged): the defaults, every schedule the GPU tests force (read as an inverse alone: SWEEP_DEBUG is no field of the
    schedule), and for a member of a merged launch MERGE_GROUP automatic and 1 .. 4"""
    out = [(tuning(), False)]
    for opts in _SCHEDULES:
        kv = {k[5:].lower(): int(v) for k, v in opts.items() if k != "GDCA_SWEEP_DEBUG"}
        assert set(kv) <= set(FIELDS), kv
        out.append((tuning(**kv), False))
    out += [(tuning(merge_group=mg), True) for mg in (-1, 1, 2, 3, 4)]
    return out


def n_reals(nblk):
    """rl = 128, 32, 16"""
    return (T * nblk, T * nblk - 100, T * nblk - 112)


def c_tuning(t):
    return (ctypes.c_int * len(FIELDS))(*[t[f] for f in FIELDS])


def new_schedule(lib, nblk, n_real, t, merged, members, timeout_ms=0):
    table = (ctypes.c_int * (3 * (nblk + 2)))()
    ints = (ctypes.c_int * 18)()
    ticks = (ctypes.c_ulonglong * 2)()
    chunks = ctypes.c_double()
    lib.schedule(nblk, n_real, CUS, c_tuning(t), timeout_ms, int(merged), members, table, ints, ticks, ctypes.byref(chunks))
    names = ("nblk", "g", "ng", "total", "total_m", "pro", "rem_tail", "ppb", "n_mcu", "mcu_solo", "ring", "slab", "n_real", "rl", "table_ints")
    s = dict(zip(names, ints[:15]))
    ng = s["ng"]
    for name, off in zip(("item0", "mitem0", "gs"), ints[15:18]):
        s[name] = list(table[off:off + ng + 1])
    assert (ints[15], ints[16], ints[17]) == (0, ng + 1, 2 * (ng + 1))  # item0 | mitem0 | gs: what k_sweep_prep copies as one block
    s["timeout_ticks"], s["hole_timeout_ticks"], s["chunks"] = ticks[0], ticks[1], chunks.value
    return s


# ---- the rules as they stood (plan_sweep before the header existed), restated -----------------------------------------------------------
def old_m_cnt(sz):
    return 1 if sz == 1 else sz * (sz + 1) + sz * (1 + SLAB_ITEMS * (sz - 1))


def old_plan(nblk, n_real, cus, t, merged, members, timeout_ms=0):
    n_pad = nblk * T
    g_merged = min(t["merge_group"], 4) if t["merge_group"] >= 1 else (4 if nblk >= 24 else (2 if nblk >= 12 else 1))
    g_rule = 4 if nblk >= 61 else (3 if nblk >= 53 else (2 if nblk >= 45 else 1))
    g = g_merged if merged else (min(t["group"], 4) if t["group"] >= 1 else g_rule)
    if nblk < 2 * g:
        g = 1
    ramp_sum = g * (g - 1) // 2
    if t["ramp"] and g > 1 and nblk >= ramp_sum + 2 * g:
        sizes = list(range(1, g))
        rest = nblk - ramp_sum
        rem = rest % g
        if rem:
            k = 0  # std::upper_bound: behind the entries <= rem
            while k < len(sizes) and sizes[k] <= rem:
                k += 1
            sizes.insert(k, rem)
        sizes += [g] * (rest // g)
    else:
        sizes = [min(g, nblk - b) for b in range(0, nblk, g)]
    ng = len(sizes)
    gs = [0]
    for sz in sizes:
        gs.append(gs[-1] + sz)
    rl = min(T, ((n_real - (nblk - 1) * T + 15) // 16) * 16) if t["ragged"] else T
    rem_tail = t["rem_tail"] if t["rem_tail"] >= 0 else (2 * cus if g >= 3 else 0)
    ppb = (2 if t["panel_halves"] else 1) if t["panel_halves"] >= 0 else (1 if g >= 3 else 2)
    single = all(sz == 1 for sz in sizes)
    slab = t["slab"] != 0 and single
    ring = min(t["ring"], 8) if single and t["ring"] >= 3 else 2
    pro = (nblk - sizes[0] - (sizes[1] if ng > 1 else 0)) * ppb * sizes[0] if ng > 0 else 0
    item0, mitem0, pos, mpos, chunks = [], [], 0, 0, 0
    for p in range(ng):
        item0.append(pos)
        mitem0.append(mpos)
        sz = sizes[p]
        nsz = sizes[p + 1] if p + 1 < ng else 0
        n2 = sizes[p + 2] if p + 2 < ng else 0
        nrest = nblk - sz - nsz
        mpos += old_m_cnt(sz) + (((SLAB_ITEMS if nsz else 0) + (2 * SLAB_ITEMS if n2 else 0)) if slab else nsz * 2 * sz + nsz * (nsz + 1) // 2)
        pos += ((2 if gs[p] + 3 < nblk else 0) + max(0, nblk - gs[p] - 4)) if slab else n2 * (n2 + 1) // 2
        pos += nsz * nrest
        pos += (nblk - sz) * sz
        pos += nrest * (nrest + 1) // 2 if nrest > 0 else 0
        pos += (nblk - nsz - n2) * ppb * nsz if nsz > 0 else 0
        pn = nblk - sz
        last = gs[p + 1] == nblk
        kch = 8 * (sz - 1) + 2 * ((rl + 31) // 32) if (rl < T and last and sz > 1) else 8 * sz
        nrag = pn if (rl < T and not last) else 0
        # (an exact sum: nrag * rl / 128 * kch is a whole number -- rl is a multiple of 16 and kch of 8)
        assert (nrag * rl * kch) % T == 0
        chunks += (pn * (pn + 1) // 2 - nrag) * kch + nrag * rl * kch // T
        chunks += pn * sz * 8 * sz
        if sz > 1:
            chunks += sz * (sz - 1) * sz * 8
    item0.append(pos)
    mitem0.append(mpos)
    model_ms = 8.0 * members * (float(n_pad) * n_pad * n_pad / 50e12 * 1e3)
    to_ms = timeout_ms if timeout_ms > 0 else max(4000, int(model_ms))
    timeout_ticks = max(1, to_ms) * 100000
    hole = min(timeout_ticks, max(50, int(model_ms)) * 100000)
    if g == 1:
        mcu_rule = 12 if nblk < 28 else 8
    else:
        mcu_rule = 16 if nblk <= 63 else (12 if nblk <= 68 else (10 if nblk <= 74 else (6 if nblk <= 90 else (4 if nblk <= 120 else 2))))
    mcu_merged = t["merge_mcus"] if t["merge_mcus"] >= 1 else min(mcu_rule, max(2, cus // (8 * max(1, members))))
    solo = (not merged) and ((t["mcu_solo"] != 0) if t["mcu_solo"] >= 0 else g in (2, 3))
    mcu_solo_rule = 12 if g == 2 else 16
    if merged:
        n_mcu = min(mcu_merged, 16)
    elif t["mcus"] >= 1:
        n_mcu = min(t["mcus"], 32 if solo else 16)
    else:
        n_mcu = mcu_solo_rule if (solo and t["mcu_solo"] < 0) else mcu_rule
    return dict(nblk=nblk, g=g, ng=ng, gs=gs, item0=item0, mitem0=mitem0, pro=pro, total=pro + pos, total_m=mpos, rem_tail=rem_tail, ppb=ppb,
                slab=SLAB_ITEMS if slab else 0, ring=ring, n_real=n_real, rl=rl, n_mcu=n_mcu, mcu_solo=1 if solo else 0,
                timeout_ticks=timeout_ticks, hole_timeout_ticks=hole, chunks=float(chunks), table_ints=3 * (ng + 1))


def test_the_schedule_is_the_rules_as_they_stood(lib):
    seen_g, seen_gm, seen_mcu = {}, {}, {}
    for nblk in NBLKS + (45, 53, 61, 63, 64, 68, 69, 74, 75, 90, 91, 120, 121):
        for n_real in n_reals(nblk):
            for t, merged in settings():
                for members in ((1, MEMBERS) if merged else (1,)):
                    got = new_schedule(lib, nblk, n_real, t, merged, members)
                    want = old_plan(nblk, n_real, CUS, t, merged, members)
                    assert got == want, (nblk, n_real, t, merged, members, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
                    if t == DEFAULTS:
                        (seen_gm if merged else seen_g)[nblk] = got["g"]
                        if not merged:
                            seen_mcu[nblk] = got["n_mcu"]
    # the boundaries of the measured rules are among the cases: the group rule, the merged rule, the ladder of chain compute units
    assert [seen_g[b] for b in (44, 45, 52, 53, 60, 61)] == [1, 2, 2, 3, 3, 4]
    assert [seen_gm[b] for b in (11, 12, 23, 24)] == [1, 2, 2, 4]
    ladder = {}
    for nblk in (63, 64, 68, 69, 74, 75, 90, 91, 120, 121):  # groups of four with two workers a unit: the rule itself
        ladder[nblk] = new_schedule(lib, nblk, T * nblk, tuning(group=4, mcu_solo=0), False, 1)["n_mcu"]
    assert [ladder[b] for b in (63, 64, 68, 69, 74, 75, 90, 91, 120, 121)] == [16, 12, 12, 10, 10, 6, 6, 4, 4, 2]
    assert [seen_mcu[b] for b in (27, 28, 64, 91, 121)] == [12, 8, 12, 4, 2]


def test_the_wait_bounds(lib):
    """the time-out model: the option, the 4-s floor, the modelled duration of what the launch carries"""
    for nblk, members, timeout_ms in ((4, 1, 0), (4, 8, 0), (157, 1, 0), (157, 8, 0), (375, 1, 0), (375, 8, 0), (79, 1, 1), (79, 1, 250), (375, 8, 60000)):
        got = new_schedule(lib, nblk, T * nblk, tuning(), members > 1, members, timeout_ms)
        want = old_plan(nblk, T * nblk, CUS, tuning(), members > 1, members, timeout_ms)
        assert (got["timeout_ticks"], got["hole_timeout_ticks"]) == (want["timeout_ticks"], want["hole_timeout_ticks"]), (nblk, members, timeout_ms)


def test_chunks_of_a_ragged_last_group(lib):
    """g_chunks, the count the kernels loop to, is the count the flop figure was built from (plan_sweep's kch)"""
    for nblk in (5, 9, 47, 64):
        for n_real in n_reals(nblk) + (T * nblk - 1, T * nblk - 127):
            for group in (1, 2, 3, 4):
                t = tuning(group=group)
                want = old_plan(nblk, n_real, CUS, t, False, 1)
                table = (ctypes.c_int * (3 * (nblk + 2)))()
                for p in range(want["ng"]):
                    sz = want["gs"][p + 1] - want["gs"][p]
                    last = want["gs"][p + 1] == nblk
                    rl = want["rl"]
                    kch = 8 * (sz - 1) + 2 * ((rl + 31) // 32) if (rl < T and last and sz > 1) else 8 * sz
                    assert lib.chunks_of_group(nblk, n_real, CUS, c_tuning(t), 0, table, p) == kch, (nblk, n_real, group, p)


def test_the_lists_cover_the_work_exactly_once(lib):
    msg = ctypes.create_string_buffer(256)
    schedules = 0
    for nblk in NBLKS:
        for n_real in n_reals(nblk):
            for t, merged in settings():
                bad = lib.coverage(nblk, n_real, CUS, c_tuning(t), int(merged), MEMBERS if merged else 1, msg, len(msg))
                assert bad == 0, (nblk, n_real, t, merged, bad, msg.value.decode())
                schedules += 1
    assert schedules == len(NBLKS) * 3 * (1 + len(_SCHEDULES) + 5)


def test_the_flag_block(lib):
    """the regions of the flag block do not overlap, in the order the kernels' descriptor names them, and end inside what the workspace
    sets aside for a matrix of that size whatever its groups (gdca_inverse_flag_bytes); the item table fits its room"""
    out = (ctypes.c_ulonglong * 14)()
    for nblk in NBLKS:
        ngs = {new_schedule(lib, nblk, T * nblk, t, merged, MEMBERS if merged else 1)["ng"] for t, merged in settings()}
        assert max(ngs) <= nblk
        for ng in sorted(ngs | {nblk}):
            lib.flags(nblk, ng, out)
            gen, rb, mc, done, sl, nxt, next_m, mxcc, arrived, mcu, abort, words, words_max, table_max = list(out)
            sizes = [(gen, nblk * nblk), (rb, ng * nblk), (mc, ng), (done, ng), (sl, 3 * ng), (nxt, 1), (next_m, 1), (mxcc, 1), (arrived, 1), (mcu, 32),
                     (abort, 1)]
            end = 0
            for off, n in sizes:
                assert off >= end, (nblk, ng, sizes)
                end = off + n
            assert end <= words <= words_max, (nblk, ng)
            # the abort word shares no 128-byte line with the counters (the block itself is 128-byte aligned or not: 32 words apart either way)
            assert abort - (mcu + 32) >= 0 and abort - nxt >= 32 and words - abort >= 32
            # what gdca_inverse_flag_bytes returned before the layout had a function: (2 nblk^2 + 5 nblk + 96) words
            assert words_max == 2 * nblk * nblk + 5 * nblk + 96
            assert 3 * (ng + 1) <= table_max
