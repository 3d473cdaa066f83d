// The schedule of the persistent SPD-inverse sweep (k_inverse.hip): which groups the pivot blocks form, the two lists of
// work items the launch hands out -- the main list and the M list (the serial chain) -- and where the dependency flags lie.  The host
// builds the lists as three small tables (sweep_schedule) and the kernels turn an item number back into what to do (main_decode; the
// chain worker's walk, stated here as chain_decode): every tile, panel half and write-back of every group has to come out exactly
// once.  Both sides are this one text -- the decode is a template over the descriptor, the kernels' SweepDesc or the host's Schedule,
// whose fields carry the same names, and the host's per-group counts are sums of the very terms the decode subtracts.  Plain C++
// without a HIP include, so that a host test (tests/test_sweep_schedule_cpu.py compiles this header alone) enumerates both lists
// and counts what they name.
#pragma once

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define GDCA_SWEEP_HD static __host__ __device__ inline __attribute__((always_inline))
#else
#define GDCA_SWEEP_HD static inline
#endif

constexpr int GDCA_SWEEP_TILE = 128;       // tile edge
constexpr int GDCA_SWEEP_KC = 16;          // k-chunk staged per pass
constexpr int GDCA_SWEEP_SLAB_ITEMS = 8;   // 16-row slabs of a 128-row block (the chain's row-slab items)
constexpr int GDCA_SWEEP_MAX_MERGE = 8;    // inverses one merged launch carries (k_sweep_merged)

namespace gdca_sweep {

GDCA_SWEEP_HD int imin(int a, int b)
{
    return a < b ? a : b;
}
GDCA_SWEEP_HD int imax(int a, int b)
{
    return a > b ? a : b;
}

// ---- the groups ----------------------------------------------------------------------------------------------------------------------
template <class Desc>
GDCA_SWEEP_HD int g_start(const Desc &D, int p)
{
    return D.gs[p];
}
template <class Desc>
GDCA_SWEEP_HD int g_size(const Desc &D, int p)
{
    return D.gs[p + 1] - D.gs[p];
}
// k-chunks (16 deep) of a tile item of update p: 8 per pivot block; the block at the ragged end of the matrix counts only the
// chunks that hold real columns (rl of its 128; the padding columns of G and H are zero), rounded up to an even number
template <class Desc>
GDCA_SWEEP_HD int g_chunks(const Desc &D, int p)
{
    const int sz = g_size(D, p);
    if (D.rl < GDCA_SWEEP_TILE && D.gs[p + 1] == D.nblk && sz > 1)
        return (GDCA_SWEEP_TILE / GDCA_SWEEP_KC) * (sz - 1) + 2 * ((D.rl + 2 * GDCA_SWEEP_KC - 1) / (2 * GDCA_SWEEP_KC));
    return (GDCA_SWEEP_TILE / GDCA_SWEEP_KC) * sz;
}
// tile and write-back items of group p (what done[p] counts up to)
template <class Desc>
GDCA_SWEEP_HD unsigned g_done_total(const Desc &D, int p)
{
    const int sz = g_size(D, p), pn = D.nblk - sz;
    return (unsigned)(pn * sz + (long long)pn * (pn + 1) / 2);
}

// M(q): sz (sz+1) / 2 gather items (one lower tile each), per block w a pivot + 8 (sz-1) row-slab jobs, then
// sz (sz+1) / 2 scatter items
// (a group of ONE block needs no scratch copy: a single item, the pivot in place)
GDCA_SWEEP_HD int m_items(int sz)
{
    return sz == 1 ? 1 : sz * (sz + 1) + sz * (1 + GDCA_SWEEP_SLAB_ITEMS * (sz - 1));
}

// ---- the sections of a group's sequence in the main list (main_decode walks them in this order; main_items is their sum) ---------------
// diag2 of the group that starts at block b0, n2 = the size of the group after the next: the tiles of that group's diagonal
// super-block -- between single blocks (slab): (b0+3, b0+3) and column b0 + 2 from row b0 + 3 down
template <class Desc>
GDCA_SWEEP_HD int n_diag2(const Desc &D, int b0, int n2)
{
    return D.slab ? (b0 + 3 < D.nblk ? 2 : 0) + imax(0, D.nblk - b0 - 4) : n2 * (n2 + 1) / 2;
}
// write-back items of a group of sz blocks
template <class Desc>
GDCA_SWEEP_HD int n_wb(const Desc &D, int sz)
{
    return (D.nblk - sz) * sz;
}
// remainder tiles: the lower triangle of the nrest blocks outside the group and the next (its diag2 tiles are empty items)
GDCA_SWEEP_HD int n_rem(int nrest)
{
    return nrest > 0 ? nrest * (nrest + 1) / 2 : 0;
}
// panel(p+1), the rows outside groups p+1 (nsz blocks) and p+2 (n2 blocks); none behind the last group (nsz = 0)
template <class Desc>
GDCA_SWEEP_HD int n_pan(const Desc &D, int nsz, int n2)
{
    return (D.nblk - nsz - n2) * D.ppb * nsz;
}
// the chain's items of row rr of the next group (no slabs): the 2 sz panel items of the row, then the tiles (rr, 0 .. rr) of its
// diagonal super-block
GDCA_SWEEP_HD int chain_row_items(int sz, int rr)
{
    return 2 * sz + rr + 1;
}

// ---- the main list: item number -> what to do --------------------------------------------------------------------------
// The first D.pro items are panel(0); then, group after group,
//     diag2(p+2) | rest(p+1) | wb(p) | rem(p) but for its tail | panel(p+1) | the tail of rem(p)
// (panel(p+1) covers the rows outside groups p+1 and p+2: Pg(p+1) comes from the chain, which runs a group ahead, and its
// other inputs were produced early in this sequence -- so the panels are complete when the tile items of update p+1 are
// handed out, instead of holding all of them up at the start of every group).
// kind 0: panel item (group p, row block a, part b); 1: tile item (group p, tile (a, b)); 4: the same, one of the early ones the
// chain of a later group waits for (diag2, rest); 2: write-back item (group p, index a); 3: nothing (a remainder slot that
// belongs to diag2).  `p` is the caller's running group (items ascend).
struct MainItem {
    int kind, p, a, b;
};
template <class Desc>
GDCA_SWEEP_HD MainItem main_decode(const Desc &D, int &p, int item)
{
    if (item < D.pro) {  // panel(0): nobody is ahead of it
        const int sz0 = g_size(D, 0), nsz0 = D.ng > 1 ? g_size(D, 1) : 0;
        const int i0 = sz0 + nsz0 + item / (D.ppb * sz0);
        if (D.slab && i0 == 2) return MainItem{3, 0, 0, 0};  // row block b0 + 2: the chain's (sweep_slab_item, rowoff 2)
        return MainItem{0, 0, i0, item % (D.ppb * sz0)};
    }
    while (item - D.pro >= D.item0[p + 1]) ++p;
    int e = item - D.pro - D.item0[p];
    const int b0 = g_start(D, p), sz = g_size(D, p), c0 = b0 + sz;
    const int nsz = p + 1 < D.ng ? g_size(D, p + 1) : 0, d0 = c0 + nsz;
    const int n2 = p + 2 < D.ng ? g_size(D, p + 2) : 0;
    const int nrest = D.nblk - sz - nsz;  // blocks outside this group and the next
    // (between single blocks the chain itself does tiles (b0+1, b0+1), (b0+2, b0+1), (b0+2, b0+2) and the panels of row blocks
    // b0 + 1 and b0 + 2 -- sweep_slab_item, sweep_xslab_item -- and what it waits for a step later is row block b0 + 3: its tiles
    // (b0+3, b0+2), (b0+3, b0+3) take the early slots here, (b0+3, b0+1) is among rest(p+1))
    // ... and the tiles (i, b0+2), i > b0+3, follow them: column b0 + 2 is the next step's column b0 + 1, whose tiles must carry
    // this update before they can take the next one early -- as ordinary remainder tiles they were what the chain ended up waiting for
    const int nd2 = n_diag2(D, b0, n2);
    if (e < nd2) {
        if (D.slab) return e < 2 ? MainItem{4, p, b0 + 3, b0 + 2 + e} : MainItem{4, p, b0 + 2 + e, b0 + 2};
        int mm = 0, first = 0;
        while (e >= first + (n2 - mm)) {
            first += n2 - mm;
            ++mm;
        }
        return MainItem{4, p, d0 + mm + (e - first), d0 + mm};
    }
    e -= nd2;
    if (e < nsz * nrest) {
        const int mm = e / nrest, local = e % nrest;
        const int b = local < b0 ? local : local - b0 + d0;
        const int cb = c0 + mm;
        if (D.slab && b == d0) return MainItem{3, p, 0, 0};  // tile (c0 + 1, c0): done on the chain (sweep_xslab_item)
        return MainItem{4, p, b > cb ? b : cb, b > cb ? cb : b};
    }
    e -= nsz * nrest;
    const int nwb = n_wb(D, sz);
    if (e < nwb) return MainItem{2, p, e, 0};
    e -= nwb;
    const int nrem = n_rem(nrest);
    const int n_head = nrem - imin(nrem, D.rem_tail);
    if (e >= n_head) {
        const int npan = nsz > 0 ? n_pan(D, nsz, n2) : 0;  // (the guard only keeps D.ppb from being read where it is not needed)
        if (e - n_head < npan) {
            const int ep = e - n_head;
            int i = ep / (D.ppb * nsz);
            if (i >= c0) i += nsz + n2;
            if (D.slab && i == c0 + 2) return MainItem{3, p, 0, 0};  // row block b0' + 2 of group p + 1 (b0' = c0): the chain's
            return MainItem{0, p + 1, i, ep % (D.ppb * nsz)};
        }
        e -= npan;
    }
    int ii = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while ((long long)ii * (ii + 1) / 2 > e) --ii;
    while ((long long)(ii + 1) * (ii + 2) / 2 <= e) ++ii;
    int jj = e - (int)((long long)ii * (ii + 1) / 2);
    if (ii >= b0) ii += sz + nsz;
    if (jj >= b0) jj += sz + nsz;
    if (D.slab) {
        // (b0+2, b0+2): the chain's; (b0+3, b0+3) and column b0 + 2 below the diagonal: early slots
        if ((jj >= d0 && ii <= d0 + 1) || jj == d0) return MainItem{3, p, 0, 0};
    } else if (jj >= d0 && ii < d0 + n2)
        return MainItem{3, p, 0, 0};  // inside the diagonal super-block of group p+2: done as diag2
    return MainItem{1, p, ii, jj};
}
// items of group p's sequence in the main list (item0[p + 1] - item0[p])
template <class Desc>
GDCA_SWEEP_HD long long main_items(const Desc &D, int p)
{
    const int sz = g_size(D, p), nsz = p + 1 < D.ng ? g_size(D, p + 1) : 0, n2 = p + 2 < D.ng ? g_size(D, p + 2) : 0;
    const int nrest = D.nblk - sz - nsz;
    return (long long)n_diag2(D, g_start(D, p), n2) + (long long)nsz * nrest + n_wb(D, sz) + n_rem(nrest) +
           n_pan(D, nsz, n2);
}

// ---- the M list (the serial chain): item number -> what to do ---------------------------------------------------------------------------
// Group after group: M(q), then the next group's panel rows and its diagonal tiles -- or, between single blocks, the fused slab items.
// kind CHAIN_M: item a of M(q); CHAIN_SLAB / CHAIN_XSLAB / CHAIN_SLAB2: slab item a of row b0 + 1 (sweep_slab_item, rowoff 1), xslab item
// a (sweep_xslab_item), slab item a of row b0 + 2 (rowoff 2); CHAIN_MPANEL: panel item of group q, row block a, half b; CHAIN_DIAG: tile
// (a, b) of update q, inside the next group's diagonal super-block.  `q` is the caller's running group (items ascend).
// The host's form: the kernels' own is the walk inside sweep_chain_worker (k_inverse.hip), the same sections in the same order on
// m_items and SLAB_ITEMS, written out there -- behind this function, or with as little as chain_row_items in its loop, hipcc compiles
// that 140-KB function to other registers and another scratch size, and the sweep's code is kept byte for byte.  The per-group count
// below (chain_items) and the CPU test read this one.
enum : int { CHAIN_M = 0, CHAIN_SLAB = 1, CHAIN_XSLAB = 2, CHAIN_SLAB2 = 3, CHAIN_MPANEL = 4, CHAIN_DIAG = 5 };
struct ChainItem {
    int kind, q, a, b;
};
template <class Desc>
GDCA_SWEEP_HD ChainItem chain_decode(const Desc &D, int &q, int item)
{
    while (item >= D.mitem0[q + 1]) ++q;
    int e = item - D.mitem0[q];
    const int b0 = g_start(D, q), sz = g_size(D, q), c0 = b0 + sz;
    const int nm = m_items(sz);
    if (e < nm) return ChainItem{CHAIN_M, q, e, 0};
    e -= nm;
    if (D.slab) {
        if (e < GDCA_SWEEP_SLAB_ITEMS) return ChainItem{CHAIN_SLAB, q, e, 0};
        if (e < 2 * GDCA_SWEEP_SLAB_ITEMS) return ChainItem{CHAIN_XSLAB, q, e - GDCA_SWEEP_SLAB_ITEMS, 0};
        return ChainItem{CHAIN_SLAB2, q, e - 2 * GDCA_SWEEP_SLAB_ITEMS, 0};
    }
    // the next group's rows, one after the other: the 2 sz panel items of row rr, then the tiles (rr, 0 .. rr) of its
    // diagonal super-block -- its FIRST diagonal tile, which the next group's first pivot waits for, is complete after one
    // round of panel items instead of after all of them
    int rr = 0;
    while (e >= chain_row_items(sz, rr)) {
        e -= chain_row_items(sz, rr);
        ++rr;
    }
    if (e < 2 * sz) return ChainItem{CHAIN_MPANEL, q, c0 + rr, e};
    e -= 2 * sz;
    return ChainItem{CHAIN_DIAG, q, c0 + rr, c0 + e};
}
// items of group p in the M list (mitem0[p + 1] - mitem0[p])
template <class Desc>
GDCA_SWEEP_HD long long chain_items(const Desc &D, int p)
{
    const int sz = g_size(D, p), nsz = p + 1 < D.ng ? g_size(D, p + 1) : 0, n2 = p + 2 < D.ng ? g_size(D, p + 2) : 0;
    long long n = m_items(sz);
    if (D.slab)
        return n + (nsz ? GDCA_SWEEP_SLAB_ITEMS : 0) + (n2 ? 2 * GDCA_SWEEP_SLAB_ITEMS : 0);
    for (int rr = 0; rr < nsz; ++rr) n += chain_row_items(sz, rr);
    return n;
}

// ---- the flag block ------------------------------------------------------------------------------------------------------------------
// word offsets of the regions of the sweep's flags (SweepDesc says what each holds):
// gen, rb (ng <= nblk), mc, done, sl | next, next_m, mxcc, arrived, mcu[32] | the abort word on a 128-byte line of its own (every wait
// of the kernel reads it; the line of the item counters is busy with atomics)
struct FlagLayout {
    size_t gen, rb, mc, done, sl, next, next_m, mxcc, arrived, mcu, abort;
    size_t words;  // the end of the block
};
static inline FlagLayout flag_layout(int nblk, int ng)
{
    FlagLayout L{};
    size_t f = 0;
    L.gen = f;
    f += (size_t)nblk * nblk;
    L.rb = f;
    f += (size_t)ng * nblk;
    L.mc = f;
    f += ng;
    L.done = f;
    f += ng;
    L.sl = f;
    f += 3 * (size_t)ng;
    L.next = f;
    L.next_m = f + 1;
    L.mxcc = f + 18;
    L.arrived = f + 19;
    L.mcu = f + 20;  // 32 slots
    L.abort = f + 64;
    L.words = f + 96;
    return L;
}
// what a workspace sets aside for the flags of a matrix of nblk blocks, whatever its groups (gdca_inverse_flag_bytes)
static inline size_t flag_words_max(int nblk)
{
    return flag_layout(nblk, nblk).words;
}

// ---- the item table ------------------------------------------------------------------------------------------------------------------
// three tables of ng + 1 ints, one behind the other: item0, mitem0, gs
static inline int table_ints(int ng)
{
    return 3 * (ng + 1);
}
static inline int table_ints_max(int nblk)  // (ng <= nblk)
{
    return table_ints(nblk);
}

// ---- the schedule --------------------------------------------------------------------------------------------------------------------
// the switches of gdca_tuning (gdca_internal.h) the schedule reads; -1 = "the measured rule" where a rule exists
struct Tuning {
    int group, ramp, ragged, rem_tail, panel_halves, slab, ring, mcus, mcu_solo, merge_group, merge_mcus;
    long sweep_timeout_ms;
};

// Everything about one inverse that follows from its size and the switches.  What the decode reads carries SweepDesc's names.
struct Schedule {
    int nblk, g, ng;
    int *gs, *item0, *mitem0;  // [ng + 1] each, in the caller's table
    int total, total_m;
    int pro, rem_tail, ppb, n_mcu, mcu_solo, ring, slab;
    int n_real, rl;
    unsigned long long timeout_ticks, hole_timeout_ticks;
    double chunks;   // 128 x 128 x 16 MFMA chunk products issued (tile, panel and super-block items)
    int table_ints;  // what of `table` was written
};

// Host side: the schedule of one inverse of nblk blocks (n_real real rows) on a device of update_cus compute units -- group sizes, the
// item table (written to `table`, table_ints_max(nblk) ints), the counts and rules of the descriptor.  `merged`: the inverse is a
// member of a merged launch of `members` families (single-block groups, chain CUs from the merge rule, no trace).
// `table` is read back a few dozen times per group (the counts go through g_size): ordinary memory -- built straight in the pinned
// staging buffer a step of config B took 10 - 15 us longer (1.464 against 1.449 ms, medians of six alternating pairs); plan_sweep copies it there.
static inline Schedule sweep_schedule(int nblk, int n_real, int update_cus, const Tuning &tu, bool merged, int members, int *table)
{
    // pivot blocks per group: more blocks per pass raise the update's arithmetic intensity (K = 128 g) and amortise the per-item
    // costs; the serial chain of a group grows with g (and has the group's whole update to hide behind).  Small matrices
    // are bound by the chain itself, which is shortest with single blocks (no scratch copy, no tile jobs).  Measured on
    // MI355X with the round-3 tile loop and chain (tools/sweep_groups.py, profiles/r03_sweep_groups*.log: inverse time over
    // N x g x chain CUs): g = 1 is fastest up to 48 blocks (beyond, its K = 128 updates are bound by the traffic of the C tiles, not
    // by the chain), 2 to 54, 3 to 57, 4 from 58 on (with the super-block inverse as row-slab jobs; as half-tile jobs its chain hid only
    // from 71 blocks).
    // A member of a merged launch: its chain hides behind the other members' tile items, so what counts is the traffic of the C
    // tiles -- groups of four from 24 blocks, of two from 12 (option GDCA_MERGE_GROUP forces a size).
    const int g_merged = tu.merge_group >= 1 ? imin(tu.merge_group, 4) : (nblk >= 24 ? 4 : (nblk >= 12 ? 2 : 1));
    // Round 5 measured the final kernel again, every block count from 44 to 77, the four sizes alternating inside one process, twice in
    // opposite order (tools/option_probe.py, profiles/r05_group_rule.log; the two passes agree to 1 %): 1 up to 46 blocks, 2 up to 53, 3 up to
    // 59, 4 from 60 (rounds 3-4: 2 from 49, 3 from 55, 4 from 58; 3-4 % at 47, 48, 54, 58 and 59 blocks) ...
    // ... and once more with one chain worker per compute unit for groups of two and three (below, profiles/r05_group_rule.log, second
    // part): 1 up to 44 blocks, 2 up to 52, 3 up to 60, 4 from 61.
    const int g_rule = nblk >= 61 ? 4 : (nblk >= 53 ? 3 : (nblk >= 45 ? 2 : 1));
    int g = merged ? g_merged : (tu.group >= 1 ? imin(tu.group, 4) : g_rule);
    if (nblk < 2 * g) g = 1;
    // group sizes.  Before the first update there is nothing to hide the first chain behind: with full groups from the start
    // every workgroup waits ~400 us (2 % of the inverse at n = 10 000) for the first super-block inverse.  So the sweep opens
    // with a ramp 1, 2, .. g-1 (a single block is one in-place pivot item, ~70 us; each following chain is as long as the
    // update before it), and the remainder of nblk / g joins the ramp instead of ending the sweep as a lone short group
    // (measured at n = 10 000: 17.9-18.1 ms against 18.2-18.3 with the remainder last and 18.2 without the ramp).
    // GDCA_RAMP=0: uniform groups, the remainder last.
    const int ramp_sum = g * (g - 1) / 2;
    const bool ramp = tu.ramp && g > 1 && nblk >= ramp_sum + 2 * g;
    const int rest = nblk - ramp_sum, rem = ramp ? rest % g : 0;
    const int ng = ramp ? (g - 1) + (rem ? 1 : 0) + rest / g : (nblk + g - 1) / g;
    // item table: item0, mitem0, gs
    int *it = table;
    int *mit = it + (ng + 1);
    int *gs = it + 2 * (ng + 1);
    gs[0] = 0;
    if (ramp) {
        int p = 0;
        for (int k = 1; k < g; ++k) {
            gs[p + 1] = gs[p] + k;
            ++p;
            if (k == rem) {  // (the remainder: behind the ramp's group of its own size)
                gs[p + 1] = gs[p] + rem;
                ++p;
            }
        }
        for (; p < ng; ++p) gs[p + 1] = gs[p] + g;
    } else {
        for (int p = 0; p < ng; ++p) gs[p + 1] = imin(gs[p] + g, nblk);
    }
    Schedule S{};
    S.nblk = nblk;
    S.g = g;
    S.ng = ng;
    S.gs = gs;
    S.item0 = it;
    S.mitem0 = mit;
    S.table_ints = table_ints(ng);
    S.n_real = n_real;
    // real rows of the last block, in 16-row MFMA blocks: the sweep treats the matrix as n rounded up to 16, not to 128 -- the
    // tile items of the last block row and the k loop over the last pivot block skip the rest of the padding (GDCA_RAGGED=0: off)
    const int rl = tu.ragged ? imin(GDCA_SWEEP_TILE, ((n_real - (nblk - 1) * GDCA_SWEEP_TILE + 15) / 16) * 16) : GDCA_SWEEP_TILE;
    S.rl = rl;
    // remainder tiles of update p listed after panel(p+1): about one round of the workgroups, so that the panels are complete
    // when the first tile items of update p+1 are handed out and the chain has had most of update p to produce Pg(p+1).
    // Only where the update hides the chain (groups of three and four): on a chain-bound matrix Pg(p+1) is late anyway and
    // workgroups parked on panel items are missing from update p (measured: config E 59.5 instead of 63.4 families/s).
    S.rem_tail = tu.rem_tail >= 0 ? tu.rem_tail : (g >= 3 ? 2 * update_cus : 0);
    // main-list panel items: one 128 x 128 item per pivot block and row where the panels are throughput (multi-block groups of
    // three and four), two 128 x 64 halves where their latency counts
    const int ppb = tu.panel_halves >= 0 ? (tu.panel_halves ? 2 : 1) : (g >= 3 ? 1 : 2);
    S.ppb = ppb;
    // single-block groups: the chain between two pivots as fused row-slab items (sweep_slab_item; GDCA_SLAB=0: panel and tile items)
    bool slab = tu.slab != 0;
    bool single = true;
    for (int p = 0; p < ng; ++p) single = single && g_size(S, p) == 1;
    slab = slab && single;
    S.slab = slab ? GDCA_SWEEP_SLAB_ITEMS : 0;
    // buffers per kind (ring_panel): eight one-panel slots between single blocks (GDCA_RING=2: two, as for multi-block groups)
    S.ring = single && tu.ring >= 3 ? imin(tu.ring, 8) : 2;
    S.pro = ng > 0 ? (nblk - g_size(S, 0) - (ng > 1 ? g_size(S, 1) : 0)) * ppb * g_size(S, 0) : 0;  // panel(0)
    long long pos = 0, mpos = 0;
    double chunks = 0.0;
    for (int p = 0; p < ng; ++p) {
        it[p] = (int)pos;
        mit[p] = (int)mpos;
        mpos += chain_items(S, p);
        pos += main_items(S, p);
        const int sz = g_size(S, p);
        const long long pn = nblk - sz;
        const bool last = gs[p + 1] == nblk;
        const int kch = g_chunks(S, p);
        const double nrag = (rl < GDCA_SWEEP_TILE && !last) ? (double)pn : 0.0;  // tile items of the ragged block row: rl / 128 of the MFMAs
        chunks += ((double)(pn * (pn + 1) / 2) - nrag + nrag * rl / GDCA_SWEEP_TILE) * kch;  // tile items
        chunks += (double)pn * sz * 8 * sz;                                    // panel items (K = 128 sz, 128 sz columns)
        if (sz > 1) chunks += (double)sz * (sz - 1) * sz * 8;  // super-block inverse: per block and other row, sz products of 128 x 128 x 128
    }
    it[ng] = (int)pos;
    mit[ng] = (int)mpos;
    S.total = S.pro + (int)pos;
    S.total_m = (int)mpos;
    S.chunks = chunks;
    // bound of one dependency wait (GDCA_SWEEP_TIMEOUT_MS; a healthy wait is microseconds).  By default it grows with the work the
    // launch holds: the early workgroups of a launch that starts behind another one (two contexts in flight on one GPU, another
    // tenant) wait for most of that launch's run time, and a slow but correct run must not be turned into GDCA_EHIP -- 4 s or
    // eight times the modelled duration of everything this launch carries (n = 48 000: 1.8 s measured), whichever is longer
    const double n_pad = (double)nblk * GDCA_SWEEP_TILE;
    const double model_ms = 8.0 * members * (n_pad * n_pad * n_pad / 50e12 * 1e3);
    const long model_l = (long)model_ms;
    const long timeout_ms = tu.sweep_timeout_ms > 0 ? tu.sweep_timeout_ms : (model_l > 4000L ? model_l : 4000L);
    S.timeout_ticks = (unsigned long long)(timeout_ms > 1L ? timeout_ms : 1L) * 100000ull;
    // ... and once a polling wave has been off the hardware (spin_until): 50 ms or that modelled duration -- a launch that merely shares
    // the device goes on within that; one that did not get all its workgroups back never does
    const unsigned long long hole_ticks = (unsigned long long)(model_l > 50L ? model_l : 50L) * 100000ull;
    S.hole_timeout_ticks = S.timeout_ticks < hole_ticks ? S.timeout_ticks : hole_ticks;
    // compute units for the M list (same measurement): a chain-bound inverse wants every parallel item of the chain served at
    // once -- the row-slab jobs of a level of a four-block group are 24 -- and once the update hides the chain the workers go
    // back to the tiles: for multi-block groups 16 CUs up to 63 blocks, 12 up to 68, 10 up to 74, 6 up to 90 (n = 10 000: 16.5 ms
    // with 6, 16.85 with 12, 20.8 with 4), 4 up to 120, 2 beyond (n = 20 000: 123.1 ms with 2, 123.75 with 4); between single blocks (a pivot and three times eight slab items per step) 12
    // CUs below 28 blocks, 8 above
    const int mcu_rule = g == 1 ? (nblk < 28 ? 12 : 8) : (nblk <= 63 ? 16 : (nblk <= 68 ? 12 : (nblk <= 74 ? 10 : (nblk <= 90 ? 6 : (nblk <= 120 ? 4 : 2)))));
    // a member of a merged launch: its own rule unless that would hand more than an eighth of the chip to the chains
    const int mcu_merged = tu.merge_mcus >= 1 ? tu.merge_mcus : imin(mcu_rule, imax(2, update_cus / (8 * imax(1, members))));
    // One chain worker per elected compute unit (its second workgroup leaves the launch at once) for groups of two and three: there a
    // pivot shared its SIMDs with a K = 256 / 384 panel or tile item of the M list on the unit's other workgroup.  Round 5, every block
    // count from 47 to 76 with alternating settings (profiles/r05_mcu_solo.log): 12 such units for groups of two (47-53 blocks: 2-12 %
    // faster than 16 units with two workers each), 16 for groups of three (54-56 blocks 3-8 %, 58-59 1 %); groups of four and the
    // fused slab items between single blocks gain nothing (and lose workers), a merged launch's members keep both.
    // (a merged launch's members: tried, no effect -- config B eight to a launch 0.444 against 0.448 ms per family)
    const bool solo = !merged && (tu.mcu_solo >= 0 ? tu.mcu_solo != 0 : (g == 2 || g == 3));
    S.mcu_solo = solo ? 1 : 0;
    const int mcu_solo_rule = g == 2 ? 12 : 16;
    S.n_mcu = merged ? imin(mcu_merged, 16) : (tu.mcus >= 1 ? imin(tu.mcus, solo ? 32 : 16) : (solo && tu.mcu_solo < 0 ? mcu_solo_rule : mcu_rule));
    return S;
}

}  // namespace gdca_sweep
