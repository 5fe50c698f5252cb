// fl_obs.hip -- host side of the observation kernels: scratch allocation, the choice of what a launch keeps in LDS
// (obs_pick_config; the carving itself is obs_layout_c in fl_obs_layout.h, shared with the kernels), the choice of a launch class
// (obs_class_holds over the rows of OBS_CLASSES, fl_obs_layout.h) and the three launch entry points.  The kernels are fl_obs_unit.hip,
// compiled once per unit of build.sh's list (one unit per runtime-carving MODE, per launch class and per split kernel), each
// instantiating fl_obs_body.h and the phase-level headers it includes (fl_obs_ctx.h, fl_obs_passb.h, fl_obs_trees.h); obs_launch
// below reaches them all: the MODEs by its list, the classes' and split kernels by the table's rows.
#include <algorithm>
#include <utility>
#include <stdio.h>
#include <string.h>

#include "../../include/flatland_hip.h"
#include "fl_obs_layout.h"
#include "fl_obs_switches.h"

int fl_obs_alloc(FlObsScratch &o, const FlDev &d, hipStream_t s, std::vector<void *> &allocs) {
    o.pred_cap = OBS_PRED_CAP;
    o.items_cap = (size_t)d.A * (o.pred_cap + 2 * OBS_FB_NB + 2);  // bucketed lists: an item sits in every time bucket it touches
    o.wl_cap = OBS_WL_HBM_ENTRIES;
    const size_t B = (size_t)d.B, BA = B * d.A;
    // every scratch array starts out zeroed: what a kernel reads of them it has written before in the same launch, but a handle's
    // behaviour must not depend on what a freed allocation of an earlier handle left in the memory it got
    if (fl_alloc_zeroed(&o.path, BA * o.pred_cap, s, allocs) != hipSuccess ||
        fl_alloc_zeroed(&o.cell_items, B * o.items_cap, s, allocs, 64) != hipSuccess ||   // (64: conflict_flags reads up to seven words behind a list)
        fl_alloc_zeroed(&o.dbg, B * 64, s, allocs) != hipSuccess || fl_alloc_zeroed(&o.bk_rel, B * (d.Rcap + 1) * OBS_BK_NB, s, allocs) != hipSuccess ||
        fl_alloc_zeroed(&o.wl, B * o.wl_cap, s, allocs) != hipSuccess || fl_alloc_zeroed(&o.label, (size_t)d.A, s, allocs) != hipSuccess ||
        fl_alloc_zeroed(&o.rowmask, BA, s, allocs) != hipSuccess || fl_alloc_zeroed(&o.cost, B, s, allocs) != hipSuccess ||
        fl_alloc_zeroed(&o.order, B, s, allocs) != hipSuccess) return FL_ERR_HIP;
    o.rows_out = nullptr; o.rows_depth = 0; o.keep_rows = 0;
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return FL_ERR_HIP;
    o.n_cu = n_cu;
    o.order_age = 0;
    return FL_OK;
}

// The launch is one workgroup per env and a CU holds one workgroup: with more envs than CUs the launch ends when the last CU has
// worked through its envs, and the envs differ (agents on the map, traffic around them) -- mean 187 us, slowest 315 us at cfg4.
// Longest first: the workgroups take the envs in descending order of what each took in the previous launch (a counting sort
// over 1024 bins by ONE workgroup; ties in any order -- the results of an env do not depend on which workgroup builds it).
__global__ __launch_bounds__(1024) void k_env_order(int B, const uint32_t *__restrict__ cost, int *__restrict__ order) {
    __shared__ unsigned int hist[1024];
    __shared__ unsigned int wsum[16];
    __shared__ unsigned int cmax;
    const int tid = threadIdx.x;
    hist[tid] = 0;
    if (tid == 0) cmax = 1;
    __syncthreads();
    unsigned int m = 0;
    for (int b = tid; b < B; b += 1024) m = max(m, cost[b]);
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned int)__shfl_down((int)m, off));
    if ((tid & 63) == 0) atomicMax(&cmax, m);
    __syncthreads();
    const unsigned long long top = cmax;
    for (int b = tid; b < B; b += 1024) atomicAdd(&hist[1023u - (unsigned int)((unsigned long long)cost[b] * 1023ull / top)], 1u);
    __syncthreads();
    // exclusive prefix over the bins (bin 0 = the longest envs)
    const unsigned int v = hist[tid];
    unsigned int incl = v;
    for (int off = 1; off < 64; off <<= 1) { const unsigned int u = (unsigned int)__shfl_up((int)incl, off); if ((tid & 63) >= off) incl += u; }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    unsigned int base = 0;
    for (int w = 0; w < (tid >> 6); w++) base += wsum[w];
    __syncthreads();
    hist[tid] = base + incl - v;
    __syncthreads();
    for (int b = tid; b < B; b += 1024) order[atomicAdd(&hist[1023u - (unsigned int)((unsigned long long)cost[b] * 1023ull / top)], 1u)] = b;
}

// FL_OBS_KEEP_VERIFY (diagnostic): FL_OBS_KEEP_TREE_ROWS rests on the caller's promise that the tree buffer is the previous launch's, untouched
// -- a buffer that was freed and re-allocated at the same address, or a tensor modified in place (-inf replaced before a network), breaks it
// silently.  With the switch set, every launch that skips the pre-fill first checks the promise: a row the masks call constant must still be
// -inf, a row they call real must not be; a violation latches FL_ERR_ARG for the env (fl_check: "tree buffer modified").
__global__ void k_keep_verify(int B, int A, int n_rows, const double *__restrict__ out, const uint4 *__restrict__ rowmask, int *__restrict__ err) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (long long)B * A * n_rows) return;
    const long long g = k / n_rows;
    const int row = (int)(k % n_rows);
    const uint4 m = rowmask[g];
    if (!m.w) return;
    const uint32_t w = row < 32 ? m.x : row < 64 ? m.y : m.z;
    const bool real = (w >> (row & 31)) & 1u;
    const double v = out[k * 12];
    const bool ninf = isinf(v) && v < 0;
    if (real == ninf) atomicCAS(&err[g / A], 0, FL_ERR_ARG);
}
static void obs_keep_verify(const FlDev &d, const ObsArgs &P, const uint4 *rowmask, hipStream_t s) {
    if (!obs_switches().keep_verify ||!P.keep_rows || !rowmask || P.n_tree_nodes > 96) return;
    const long long n = (long long)d.B * d.A * P.n_tree_nodes;
    hipLaunchKernelGGL(k_keep_verify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d.B, d.A, P.n_tree_nodes, P.tree_out, rowmask, d.err);
}

#ifndef OBS_ROUND16_DEFAULT
#define OBS_ROUND16_DEFAULT 0   // rounds of 16 agents on 512 threads, two workgroups a CU (MODE 5) for envs of more than 32 agents
#endif
#ifndef OBS_ORDER_EVERY
#define OBS_ORDER_EVERY 4   // what an env takes changes slowly from step to step: the order of every fourth launch serves the next three
#endif
FlObsScratch fl_obs_env_order(FlObsScratch &o, const FlDev &d, hipStream_t s) {
    FlObsScratch u = o;
    if (obs_switches().no_order || d.B <= o.n_cu) { u.order = nullptr; return u; }
    if (o.order_age++ % OBS_ORDER_EVERY == 0) hipLaunchKernelGGL(k_env_order, dim3(1), dim3(1024), 0, s, d.B, o.cost, o.order);
    return u;
}

// carve the dynamic LDS of a launch (obs_layout_c in fl_obs_layout.h: one function for the host and for the kernels with a
// compile-time layout)
static ObsLayout obs_layout(const FlDev &d, const ObsArgs &P, const ObsOptions &o) {
    return obs_layout_c(ObsDims{d.Rcap, d.A, d.Ucap, d.rkey != nullptr}, ObsShape{P.merged, P.tw_c, P.tw_t, P.tpw_t, P.tree_pred}, o);
}

// ---- the launch classes (OBS_CLASSES in fl_obs_layout.h: one row a class, compile-time carving): does class `c` hold this batch?
//   OBS_FIT_EXACT  the whole batch fits the class's capacities and the configuration just chosen for it (`own`) has the class's options
//   OBS_FIT_BIN    (round 6) the whole batch fits, and its own choice only has the class's STRUCTURE (one round / rounds of 32 agents / two
//                  stages): the class's options then REPLACE the batch's own, in P too -- a compile-time carving with the options of the
//                  bin's largest shape instead of the runtime carving with options chosen for this one (per shape of the Round-2 table:
//                  profiles/r06_round2_classes.txt).  FL_OBS_NO_BINS: exact classes only
//   OBS_FIT_SPLIT  everything but the rail cells of the batch's LARGEST map matches, and the runtime configuration chosen for the batch (L)
//                  runs the class's MODE, VAR and threads: the class's split kernel serves the envs that fit it (obs_split_count)
// EXACT and BIN: L becomes the class's carving (what the kernel has compiled in) with the next-hop tables, last in it, at the batch's size.
enum ObsFit { OBS_FIT_EXACT, OBS_FIT_BIN, OBS_FIT_SPLIT };
static int obs_var(const ObsLayout &L) { return L.tab_lds ? 1 : L.wl_bytes == 0 ? 2 : 0; }
static bool obs_class_holds(const ObsClass &c, ObsFit kind, const FlDev &d, ObsArgs &P, const ObsOptions &own, ObsLayout &L) {
    const ObsLayout &CL = OBS_CLASS_LAYOUTS.L[&c - OBS_CLASSES];
    if (c.opt.wl_head && obs_switches().no_wl_head) return false;
    if (P.label) return false;   // (get_many(handles) with a strict subset: the stand-alone kernel's runtime body)
    if (P.keep_mode && !c.keep_rows) return false;   // (FL_OBS_KEEP_TREE_ROWS: the runtime carving instead)
    if (!P.compact_t || (d.rkey != nullptr) != (c.dims.rkey != 0) || (c.agents != 0 ? d.A != c.agents : d.A > c.dims.A)) return false;
    if (P.merged != c.shape.merged || P.tw_c != c.shape.tw_c || P.tw_t != c.shape.tw_t || P.tpw_t != c.shape.tpw_t) return false;
    // the class's kernel has the builders' parameters compiled in
    if (P.max_nodes != c.max_nodes || P.pred_depth != c.pred_depth || P.tree_pred != c.shape.tree_pred || (c.max_depth != 0 && P.max_depth != c.max_depth)) return false;
    if (c.opt.dual && (size_t)d.A * (P.tree_pred + 2) > (size_t)CL.items2_cap) return false;
    const size_t total = c.opt.nh ? CL.off[L_NH] + obs_al16((unsigned long long)d.Ucap * d.Rcap * 2) : CL.total;
    if (total > (size_t)160 * 1024) return false;
    switch (kind) {
    case OBS_FIT_SPLIT:   // (no options compared: the class's body has its own compiled in; the rail cells are counted per env)
        return obs_var(L) == obs_class_var(c) && L.nt == c.opt.nt;
    case OBS_FIT_EXACT:
        // ... and what the launcher derives from the options: the kernel has the class's values (obs_class_* in fl_obs_layout.h)
        if (d.Rcap > c.dims.Rcap || !obs_same_options(own, c.opt)) return false;
        if (P.bk != obs_class_bk(c) || P.wl_occ_div != obs_class_wl_occ_div(c) || P.tshift != obs_class_tshift(c, d.A)) return false;
        break;
    case OBS_FIT_BIN:
        if (d.Rcap > c.dims.Rcap) return false;
        // the large-map bins have no LDS successor table: not for a batch that affords one itself (Test_12: 200 agents on 2 745 rail cells --
        // same box, its envs beyond class 4 on the runtime carving WITH the table 435 us, on class 14 without 442)
        if (!c.opt.snext && c.dims.rkey == 0 && own.snext) return false;
        if (c.shape.tw_t != 0 && (P.max_depth < 1 || P.max_depth > 3)) return false;
        if (c.shape.merged != 0 && (long long)d.A * (P.pred_depth + 2) >= 65536) return false;
        P.use_tmask = c.opt.tmask; P.dual_index = c.opt.dual; P.bk = obs_class_bk(c);
        P.bk_nb = c.shape.merged != 0 ? OBS_FB_NB : OBS_BK_NB; P.bk_shift = c.shape.merged != 0 ? OBS_FB_SHIFT : OBS_BK_SHIFT;
        P.wl_occ_div = obs_class_wl_occ_div(c); P.tshift = obs_class_tshift(c, d.A);
        break;
    }
    L = CL;
    L.total = (unsigned)total;
    return true;
}
// the envs that class `c`'s split kernel would serve with the class's body, the others running the carving L (h_R: the host's copy of
// the envs' rail cells, null: unknown, no split); 0: no split launch of this class
static int obs_split_count(const ObsClass &c, const FlDev &d, ObsArgs &P, const ObsLayout &L, const int *h_R) {
    ObsLayout cur = L;
    if (!h_R || !obs_class_holds(c, OBS_FIT_SPLIT, d, P, ObsOptions(), cur)) return 0;
    int n = 0;
    for (int b = 0; b < d.B; b++) n += h_R[b] <= c.dims.Rcap;
    return n;
}
// the first class of `ids` (an OBS_ORDER_* list) that holds the batch becomes P.fix
static bool obs_take_first(const int *ids, ObsFit kind, const FlDev &d, ObsArgs &P, const ObsOptions &o, ObsLayout &L) {
    for (; *ids; ids++)
        if (obs_class_holds(OBS_CLASSES[obs_class_index(*ids)], kind, d, P, o, L)) { P.fix = *ids; return true; }
    return false;
}
// the launch class of a configuration just accepted (P.fix_allowed: no switch rules the classes out; which switches rule out what: fl_obs_switches.h)
static void obs_take_fixed_class(const FlDev &d, ObsArgs &P, const ObsOptions &o, ObsLayout &L) {
    P.fix = 0; P.split = 0;
    if (!P.fix_allowed) return;
    if (P.tw_t == 0) {   // the flatland_cutils builder alone
        // (FL_OBS_NO_CUTILS_MERGE, !P.cutils_alone: no bin -- but the exact classes are tried all the same, so class 9, the stand-alone kernel's, is still taken)
        if (!obs_take_first(OBS_ORDER_ALONE_EXACT, OBS_FIT_EXACT, d, P, o, L) && obs_switches().bins_allowed && P.cutils_alone) obs_take_first(OBS_ORDER_ALONE_BIN, OBS_FIT_BIN, d, P, o, L);
        return;
    }
    if (obs_take_first(OBS_ORDER_BOTH_EXACT, OBS_FIT_EXACT, d, P, o, L) || !obs_switches().bins_allowed) return;
    // an exact class's SPLIT launch (its body for the envs that fit, the runtime carving L for the few larger maps) goes before a bin class for
    // the whole batch when at least half the envs fit the exact class: no class here, obs_take_split_class takes it
    if (!obs_switches().no_split && P.h_R)
        for (const int *k = OBS_ORDER_BOTH_SPLIT_FIRST; *k; k++)
            if (2 * obs_split_count(OBS_CLASSES[obs_class_index(*k)], d, P, L, P.h_R) >= d.B) return;
    obs_take_first(OBS_ORDER_BOTH_BIN, OBS_FIT_BIN, d, P, o, L);
}

// The split launch of a configured batch (P.L, P.fix; ObsArgs::fix_allowed: chosen without the diagnostic overrides that rule the launch
// classes out).  Per workgroup the class's body for an env that fits its rail cells (d.R[b] <= dims.Rcap) and for the others
//   split 1: the runtime-carving body (P.L, unchanged) -- for a batch that no class holds whole
//   split 2: the body of the class's larger partner (`split2`: no LDS successor table), which was taken because of the batch's largest map --
//            one kernel, every env on a compile-time carving
// Returns the number of envs that fit (0: no split launch).
static int obs_take_split_class(const FlDev &d, ObsArgs &P, const int *h_R) {
    if (obs_switches().no_split || !P.fix_allowed) return 0;
    auto take = [&](const ObsClass &c, int split) {
        const int n = obs_split_count(c, d, P, P.L, h_R);
        if (n > 0) {
            P.fix = c.id; P.split = split;
            P.L.total = std::max(P.L.total, OBS_CLASS_LAYOUTS.L[&c - OBS_CLASSES].total);   // dynamic LDS of the launch: the larger of the two carvings
        }
        return n;
    };
    if (P.fix != 0) {
        for (const ObsClass &c : OBS_CLASSES)
            if (c.split2 == P.fix) return take(c, 2);
        return 0;
    }
    for (const int *k = P.tw_t == 0 ? OBS_ORDER_SPLIT_ALONE : OBS_ORDER_SPLIT_BOTH; *k; k++)
        if (const int n = take(OBS_CLASSES[obs_class_index(*k)], 1)) return n;
    return 0;
}

// ---- obs_pick_config: choose what lives in LDS so that the workgroup fits 160 KiB.  Two preference walks -- the one-pass kernels' (P.merged
// 1 / 2 / 3), then the two-stage kernels' -- and one acceptance, obs_accept, of what either of them finds.
static bool obs_ok(int forced, int v) { return forced < 0 || forced == v; }   // FL_OBS_FORCE (ObsSwitches::force): only configurations with these values
static bool obs_nh_fit(const FlDev &d) { return (size_t)d.Ucap * d.Rcap * 2 <= 24 * 1024; }  // beyond that the next-hop tables stay in HBM / L2
static bool obs_dual_ok(const FlDev &d, const ObsArgs &P) { return P.tw_c != 0 && P.tw_t != 0 && P.tree_pred >= 0 && (long long)d.A * (P.pred_depth + 2) < 65536 && (long long)d.A * (P.tree_pred + 2) < 32768; }
// what the launcher derives from the options of a configuration, where the walks differ (tshift: unless FL_OBS_TSHIFT sets it; tab_of_layout: the
// static tables joined the carving behind the options' back, so `accepted.tab` is the layout's)
struct ObsDerived { int bk, bk_nb, bk_shift, wl_occ_div, tshift; bool tab_of_layout; };
// The configuration (o, L) is chosen.  `accepted`: its options (what the launch's record and FL_OBS_VERBOSE report), untouched when nothing fits;
// what it sets in P; and the fixed launch class that has exactly these options (or whose bin holds them), if the batch fits one.
static bool obs_accept(const FlDev &d, ObsArgs &P, ObsOptions &accepted, const ObsOptions &o, ObsLayout L, const ObsDerived &v) {
    accepted = o; if (v.tab_of_layout) accepted.tab = L.tab_lds;
    P.use_tmask = o.tmask; P.dual_index = o.dual;
    P.bk = v.bk; P.bk_nb = v.bk_nb; P.bk_shift = v.bk_shift; P.wl_occ_div = v.wl_occ_div;
    P.tshift = obs_switches().tshift >= 0 ? (int)obs_switches().tshift : v.tshift;
    P.fix_allowed = obs_switches().classes_allowed;
    obs_take_fixed_class(d, P, o, L);
    P.L = L;
    return true;
}

struct ObsPref { int fb, wl, items; };
// Both builders: ONE pass B per round of 32 agents over the trees of both (trees_merged).  It needs compact upstream
// trees, sixteen wavefronts, the second index with its items and the time masks in LDS, the successor table and keys =
// rail indices (the fast classify loop).  Small envs (one round) also get the own-path filter of the classify loop.
static bool obs_walk_one_pass(const FlDev &d, ObsArgs &P, ObsOptions &accepted) {
    const ObsSwitches &sw = obs_switches();
    const bool nh_fit = obs_nh_fit(d), up = P.tw_t != 0;
    // the flatland_cutils builder ALONE on the one-pass kernels (MODE 6 / 7 / 8: no second index, no upstream tables): 32-slot trees,
    // every agent listed (get_many(handles) with a strict subset stays on the stand-alone kernel)
    const bool merge_ok = up ? obs_dual_ok(d, P) : (P.cutils_alone && P.tw_c == N_WORDS_C * OBS_CAP_C && P.label == nullptr && (long long)d.A * (P.pred_depth + 2) < 65536);
    // Rounds of 16 agents on 512 threads and at most 80 KB of LDS (MODE 5): a CU then holds TWO workgroups, and one env's barriers
    // and L2 round trips are filled by the other's issue.  FL_OBS_ROUND16=0 / 1 overrides the default.
    // Envs of at most 32 agents (rounds of 16 instead of the one-round kernel): when the batch has several envs per CU (P.wide) -- same-box
    // sweep at the cfg2 shape, runtime carving on both sides: 512 envs +7 %, 1024 +13 %, 2048 +17 % with two workgroups a CU; at one
    // env per CU the 512-thread workgroup alone takes 75 us against 53 (profiles/r05_cfg2_bsweep.json).  FL_OBS_ROUND16=2 forces it
    // for any batch, =0 rules it out.
    const bool r16_small = d.A <= 32 && (sw.round16 >= 0 ? sw.round16 == 2 : P.wide != 0);
    // ... and, round 6, envs of more than 32 agents when the builder runs ALONE on small maps (cfg3's kind) in a wide batch: without the second index
    // and the upstream tables its LDS lists and items fit 80 KB (class 21; same box at 1 024 cfg3 envs, runtime carving: 0.467 -> 0.419 ms)
    // (only where class 21 holds the batch: beyond its capacities the one-a-CU bin classes are the better choice)
    const bool r16_alone = !up && P.cutils_alone && d.A > 32 && P.wide != 0 && d.Rcap <= ObsFixed<21>::dims.Rcap && d.A <= ObsFixed<21>::dims.A;
    const bool r16 = (r16_small || (d.A > 32 && (sw.round16 >= 0 ? sw.round16 != 0 : (OBS_ROUND16_DEFAULT != 0 || r16_alone)))) && (!sw.nt || sw.nt == 512) && obs_ok(sw.force.nt, 512);
    const size_t merged_limit = r16 ? std::min((size_t)sw.lds_limit, (size_t)80 * 1024) : (size_t)sw.lds_limit;
    if (!(!sw.no_merge && merge_ok && P.compact_t && d.rkey == nullptr && (r16 || ((!sw.nt || sw.nt == OBS_NT) && obs_ok(sw.force.nt, OBS_NT))) &&
          obs_ok(sw.force.tmask, 1) && obs_ok(sw.force.dual, up ? 1 : 0) && obs_ok(sw.force.snext, 1) &&
          (!up || (size_t)d.A * (P.tree_pred + 2) <= OBS_ITEMS2_CAP))) { P.merged = 0; return false; }
    P.merged = r16 ? 3 : d.A <= 32 ? 1 : 2;
    ObsOptions o = {};
    o.nt = r16 ? 512 : OBS_NT; o.tmask = 1; o.dual = up ? 1 : 0; o.snext = 1; o.partial = 1; o.tab = 0; o.bk_room = 0;
    // Order of preference, from same-box sweeps (tools/gpu_env_sweep.sh).  One round (at most 32 agents, cfg2): 24 KB of LDS work
    // lists, the items in LDS, plain lists (the extra counting pass of the bucketed lists costs more than their short scans
    // save: 57.9 against 51.8 us).  Rounds of 32 agents: a round of 64 trees meets thousands of occupied cells, and a work
    // list that overflows is handled cell by cell inside the classify loop (cfg3: 1.04 ms with 24 KB, 0.82 ms with 36 KB) -- so
    // 36 KB of LDS lists, or else the lists in HBM scratch (no cap); the items in LDS before anything else (cfg4: 0.45 against
    // 0.52 ms); lists grouped by 32-step time buckets where their offsets fit too (cfg4: 0.48 -> 0.45 ms, cfg3 neutral).
    static const std::initializer_list<ObsPref> one_round = {{0, 24 * 1024, 1}, {0, 16 * 1024, 1}, {0, 0, 1}, {0, 24 * 1024, 0}, {0, 0, 0}, {0, 8 * 1024, 0}};
    // (round 5) HBM lists without the LDS copy of the items BEFORE the copy: at 80 agents on 60 x 60 every env has more items than the
    // 4 096 entries that fit beside the rest (the copy is dead weight there), and what it occupied becomes the lists' LDS head
    static const std::initializer_list<ObsPref> rounds = {{1, 36 * 1024, 1}, {0, 36 * 1024, 1}, {1, 0, 0}, {1, 0, 1}, {0, 0, 1}, {1, 24 * 1024, 1}, {0, 24 * 1024, 1},
                                     {0, 0, 0}, {0, 24 * 1024, 0}, {0, 8 * 1024, 0}};
    // rounds of 16 agents in 80 KB: half the trees a round meet half the cells -- 16 KB of LDS lists, else HBM scratch
    static const std::initializer_list<ObsPref> rounds16 = {{1, 16 * 1024, 1}, {0, 16 * 1024, 1}, {1, 0, 1}, {1, 12 * 1024, 1}, {0, 12 * 1024, 1}, {0, 0, 1}, {1, 16 * 1024, 0}, {1, 0, 0}, {0, 16 * 1024, 0},
                                       {0, 0, 0}, {0, 8 * 1024, 0}};
    // ... of small envs (17 .. 32 agents, two rounds): plain lists like the one-round kernel, so that the own-path filter fits too
    static const std::initializer_list<ObsPref> rounds16_small = {{0, 16 * 1024, 1}, {0, 12 * 1024, 1}, {1, 16 * 1024, 1}, {0, 0, 1}, {0, 16 * 1024, 0}, {0, 0, 0}, {0, 8 * 1024, 0}};
    for (const ObsPref &pref : P.merged == 1 ? one_round : P.merged == 2 ? rounds : d.A <= 32 ? rounds16_small : rounds16) {
        // the builder alone has the room for 36 KB of LDS lists AND the items' copy on maps where both builders never had it -- but there
        // (cfg4: 649 rail cells) every env has more items than the copy holds and the lists' entries are many: same box, runtime carving,
        // 0.268 ms with the LDS lists against 0.261 with HBM lists behind a 16 KB LDS head.  Small maps (cfg3) keep the LDS lists.
        if (!up && P.merged == 2 && pref.wl >= 36 * 1024 && d.Rcap > OBS_ALONE_LDS_LISTS_RCAP) continue;
        o.fb = pref.fb && P.pred_depth + 1 > 64; o.wl_bytes = pref.wl; o.items = pref.items;
        // diagnostic: the env's static tables in LDS too -- but never for both builders in rounds of 16 agents (MODE 5 has no VAR 1 kernel:
        // fl_obs_unit.hip), where FL_OBS_FORCE=tab=1 leaves the tables in HBM / L2
        o.tab = sw.force.tab == 1 && o.wl_bytes && nh_fit && !(P.merged == 3 && up);
        if ((o.fb && sw.no_fb) || !obs_ok(sw.force.wl, o.wl_bytes) || !obs_ok(sw.force.items, o.items) || (o.items && d.A * 32 > OBS_ITEMS_LDS_CAP)) continue;
        // the own-path filter of the classify loop (a second set of time masks) before the full-size LDS copy of the items: on
        // sparse maps a third of the conflict entries are the walking agent's own prediction (cfg4: 34 %), and an env whose
        // items do not fit the smaller copy scans them in HBM scratch at nearly the same speed
        static const int caps[3] = {OBS_ITEMS_LDS_CAP, 4096, 2048};   // (2048: cfg3 0.86 against 0.77 ms -- most envs' items then sit in HBM; only in 80 KB)
        for (o.own_filter = sw.no_own_filter ? 0 : 1; o.own_filter >= 0; o.own_filter--)
            for (int ck = 0; ck < (o.items ? (P.merged == 3 ? 3 : 2) : 1); ck++)
                for (o.raw = o.own_filter; o.raw >= 0; o.raw--)
                    for (o.nh = nh_fit ? 1 : 0; o.nh >= 0; o.nh--) {
                        if (!obs_ok(sw.force.nh, o.nh)) continue;
                        o.items_cap = caps[ck]; o.wl_head = 0;
                        ObsLayout L = obs_layout(d, P, o);
                        if (L.total > merged_limit) continue;
                        if (o.wl_bytes == 0 && !sw.no_wl_head) {   // lists in HBM scratch: an LDS head of what the carving leaves
                            const size_t room = (merged_limit - L.total) & ~(size_t)1023;
                            o.wl_head = (int)std::min(room, (size_t)OBS_WL_HEAD_MAX); if (o.wl_head < OBS_WL_HEAD_MIN) o.wl_head = 0;
                            if (o.wl_head) L = obs_layout(d, P, o);
                        }
                        // small envs: 4-step buckets (same-box A/B on cfg2: 54.8 us against 55.1 with 2-step and 56.9 with 8-step buckets)
                        return obs_accept(d, P, accepted, o, L, {o.fb ? 2 : 0, OBS_FB_NB, OBS_FB_SHIFT, d.A <= 32 ? OBS_WL_OCC_DIV : 3, d.A <= 31 ? 2 : OBS_TSHIFT, false});
                    }
    }
    P.merged = 0;
    return false;
}
// The two-stage kernels.  Order of preference, from same-box A/B runs (tools/obs_sweep.py): the most wavefronts; the full work-list space; the LDS
// copy of the items, the time masks and the second index; the successor table; the next-hop tables; own scan scratch.
// The env's distance / segment / eight-hop tables join them when there is room left (small maps): they make no
// difference in time (their gathers hit L2 and hide behind the rest) but replace narrow HBM gathers with one coalesced read.
static bool obs_walk_two_stage(const FlDev &d, ObsArgs &P, ObsOptions &accepted) {
    const ObsSwitches &sw = obs_switches();
    static const int opts[5][3] = {{1, 1, 1}, {1, 0, 1}, {1, 0, 0}, {0, 0, 1}, {0, 0, 0}};  // masks, second index, items
    const size_t lds_limit = (size_t)sw.lds_limit;
    const bool nh_fit = obs_nh_fit(d), dual_ok = obs_dual_ok(d, P);
    ObsOptions o = {};
    for (const int nt : {OBS_NT, 512, 256}) {
        o.nt = nt;
        if ((sw.nt && o.nt != sw.nt) || !obs_ok(sw.force.nt, o.nt)) continue;
        // work lists: in LDS when everything else fits beside them (small maps), else in HBM scratch (the LDS goes to the time
        // masks, the items and the second index; no cap on the entries), else LDS lists with whatever still fits
        for (int wk = 0; wk < 4; wk++) {
            o.wl_bytes = wk == 0 || wk == 2 ? 24 * 1024 : wk == 1 ? 0 : 8 * 1024;
            for (int opt = 0; opt < (wk == 0 ? 1 + !dual_ok : 5); opt++) {
                o.tmask = opts[opt][0]; o.dual = opts[opt][1]; o.items = opts[opt][2];
                if (o.dual && !dual_ok) continue;
                if (o.items && d.A * 32 > OBS_ITEMS_LDS_CAP) continue;  // hundreds of agents: their items never fit the LDS copy
                if (!obs_ok(sw.force.wl, o.wl_bytes) || !obs_ok(sw.force.tmask, o.tmask) || !obs_ok(sw.force.dual, o.dual) || !obs_ok(sw.force.items, o.items)) continue;
                // large maps: the cutils index grouped by time bucket, counted in the node tables' LDS (room for the counters)
                const bool want_bk = !sw.no_bk && o.wl_bytes == 0 && !o.items && o.tmask && !o.dual && P.tw_c != 0 && P.pred_depth + 1 > 64 &&
                                     d.A * ((1 << OBS_BK_SHIFT) + 2) <= 65535;   // (offsets inside a bucket are 16 bits)
                for (o.bk_room = want_bk ? 1 : 0; o.bk_room >= 0; o.bk_room--)
                for (o.snext = 1; o.snext >= 0; o.snext--)
                    for (o.nh = nh_fit ? 1 : 0; o.nh >= 0; o.nh--)
                        for (o.partial = 1; o.partial >= 0; o.partial--) {  // 4 KB of scan scratch: borrowed when tight
                            if (!obs_ok(sw.force.snext, o.snext) || !obs_ok(sw.force.nh, o.nh)) continue;
                            ObsLayout L = obs_layout(d, P, o);
                            if (L.total > lds_limit) continue;
                            if (sw.force.tab != 0 && nh_fit && o.wl_bytes) {   // the static tables join the carving where they fit beside it
                                ObsOptions ot = o; ot.tab = 1;
                                const ObsLayout Lt = obs_layout(d, P, ot);
                                if (Lt.total <= lds_limit) L = Lt;
                                else if (sw.force.tab == 1) continue;
                            } else if (sw.force.tab == 1) continue;
                            // 2-step buckets where the traffic is and one catch-all bucket for late times (8-step buckets over the
                            // whole horizon measured slower on every map size)
                            return obs_accept(d, P, accepted, o, L, {o.bk_room, OBS_BK_NB, OBS_BK_SHIFT, OBS_WL_OCC_DIV, OBS_TSHIFT, true});
                        }
            }
        }
    }
    return false;
}
static bool obs_pick_config(const FlDev &d, ObsArgs &P, ObsOptions &accepted) { return obs_walk_one_pass(d, P, accepted) || obs_walk_two_stage(d, P, accepted); }

static void obs_verbose(const ObsArgs &P) {
    static int printed = 0;
    const ObsLayout &L = P.L;
    if (obs_switches().verbose && printed < 4) {
        printed++;
        fprintf(stderr, "[fl_obs] fixed launch class %d%s, %d threads, %u B LDS: static tables in LDS %d, next-hop in LDS %d, successor table %d, work lists %d B, time masks %d, second index %d, items in LDS %d, one pass B for both builders %d, compact upstream trees %d, bucketed index %d\n",
                P.fix, P.split ? " (split: the envs that fit it)" : "", L.nt, L.total, L.tab_lds, L.off[L_NH] != L_ABSENT, L.off[L_SNEXT] != L_ABSENT, L.wl_bytes, P.use_tmask, P.dual_index, L.off[L_ITEMS] != L_ABSENT, P.merged, P.compact_t, P.bk);
    }
}
// one pass B (P.merged 1 / 2 / 3): MODE 3 / 4 / 5 for both builders, 6 / 7 / 8 for the flatland_cutils builder alone; else the builders of the launch
static int obs_mode(const ObsArgs &P) { return P.merged ? (P.tw_t ? 2 : 5) + P.merged : P.tw_c == 0 ? 1 : P.tw_t ? 2 : 0; }

// The kernel of a launch: the split kernel of (P.split, P.fix), the kernel of class P.fix, or else the runtime-carving kernel of the launch's
// MODE; FL_ERR_ARG for a (split, class) pair that has no kernel.  The kernels a row of OBS_CLASSES names are build.sh's units fK, sK and sKb.
template <int ROW>
static int obs_launch_row(const FlDev &d, const FlObsScratch &u, const ObsArgs &P, hipStream_t s) {
    constexpr ObsClass c = OBS_CLASSES[ROW];
    if (P.split == 2) { if constexpr (c.split2 != 0) return fl_obs_launch_class<c.id, c.split2>(d, u, P, s); else return FL_ERR_ARG; }
    if (P.split) { if constexpr (c.split_rt != 0) return fl_obs_launch_class<c.id, 0>(d, u, P, s); else return FL_ERR_ARG; }
    return fl_obs_launch_class<c.id>(d, u, P, s);
}
template <int... ROW>
static int obs_launch_class(std::integer_sequence<int, ROW...>, const FlDev &d, const FlObsScratch &u, const ObsArgs &P, hipStream_t s) {
    int rc = FL_ERR_ARG;
    (void)((P.fix == OBS_CLASSES[ROW].id && (rc = obs_launch_row<ROW>(d, u, P, s), true)) || ...);
    return rc;
}
template <int... M>
static int obs_launch_mode(int mode, const FlDev &d, const FlObsScratch &u, const ObsArgs &P, hipStream_t s) {
    int rc = FL_ERR_ARG;
    (void)((mode == M && (rc = fl_obs_launch_mode<M>(obs_var(P.L), d, u, P, s), true)) || ...);
    return rc;
}
static int obs_launch(const FlDev &d, const FlObsScratch &u, const ObsArgs &P, hipStream_t s) {
    if (P.fix) return obs_launch_class(std::make_integer_sequence<int, OBS_N_CLASSES>(), d, u, P, s);
    return P.split ? FL_ERR_ARG : obs_launch_mode<0, 1, 2, 3, 4, 5, 6, 7, 8>(obs_mode(P), d, u, P, s);
}
// the record of a launch (fl_obs.h lists the words): the ObsArgs that were launched and the options `q` the preference walk accepted for them
static void obs_record_launch(const ObsArgs &P, const ObsOptions &q, int record[FL_OBS_LAUNCH_WORDS]) {
    const ObsClass *c = P.fix ? &OBS_CLASSES[obs_class_index(P.fix)] : nullptr;
    const int rec[FL_OBS_LAUNCH_WORDS] = {c ? obs_class_mode(*c) : obs_mode(P), c ? obs_class_var(*c) : obs_var(P.L), P.fix, P.split, P.split == 2 ? c->split2 : 0, P.L.nt, (int)P.L.total,
                                          q.wl_bytes, q.tab, q.nh, q.tmask, q.dual, q.items, q.items_cap, q.snext, q.partial, q.bk_room, q.own_filter, q.fb, q.raw, q.wl_head,
                                          P.bk, P.tshift, P.compact_t, P.label != nullptr};
    memcpy(record, rec, sizeof rec);
}

// ---- what a launch asks for: the two builders' sides of the ObsArgs (the launches below and the diagnostic fl_obs_config_of_fused)
static void obs_cutils_args(ObsArgs &P, int max_nodes, int pred_depth, int wide) {
    P.max_nodes = max_nodes; P.pred_depth = pred_depth; P.wide = wide;
    P.tw_c = N_WORDS_C * (max_nodes > OBS_CAP_C ? 64 : OBS_CAP_C);   // (more than 32 nodes: 64-slot tables, one tree a wavefront -- the builder alone only)
}
// The builder alone -- what the reference's solution launches (solution/eval_env.py:15-17) -- runs on the one-pass kernels' machinery
// (MODE 6 / 7 / 8 = MODE 3 / 4 / 5 without the upstream builder; classes 6 .. 10) wherever those apply: 16-lane pass A teams need grids
// whose cells have at most two transitions a direction (every Flatland rail cell type).  FL_OBS_NO_CUTILS_MERGE: the stand-alone kernel.
static void obs_alone_args(const FlDev &d, ObsArgs &P) {
    P.compact_t = d.max_branch <= 2 && !obs_switches().no_compact;
    P.cutils_alone = !obs_switches().no_cutils_merge;
}
// node tables of the upstream builder: compact slots when no direction of a cell of the batch has more than two transitions
static void obs_tree_args(const FlDev &d, ObsArgs &P, int max_depth, int tree_pred, double *tree_out) {
    P.max_depth = max_depth; P.tree_pred = tree_pred; P.tree_out = tree_out;
    int n = 0, p = 1;
    for (int k = 0; k <= max_depth; k++) { n += p; p *= 4; }
    P.n_tree_nodes = n;
    P.compact_t = d.max_branch <= 2 && !obs_switches().no_compact;
    if (P.compact_t && max_depth >= 4) { P.tw_t = N_WORDS_T * 32; P.tpw_t = 2; }   // depth 4: 30 compact slots on a 32-lane team (the stand-alone tree launch)
    else if (P.compact_t) { P.tw_t = N_WORDS_T * OBS_CAP_T_COMPACT; P.tpw_t = 4; }
    else { P.tw_t = max_depth <= 2 ? N_WORDS_T * 32 : N_WORDS_T * 88; P.tpw_t = max_depth <= 2 ? 2 : 1; }
}
static void obs_out_args(ObsArgs &P, const FlObsScratch &o, const FlObsCutilsOut &out) {
    P.attr = out.attr; P.forest = out.forest; P.adjacency = out.adjacency; P.node_order = out.node_order; P.edge_order = out.edge_order;
    P.valid = out.valid; P.props = out.props; P.dbg = o.dbg;
}
// The configuration of a request: the preference walk, then the split class (h_R: the envs' rail cells, null: no split).  Returns how many envs
// run a launch class's body (all of them, those that fit a split class, or 0: the runtime carving), -1: no configuration fits.
static int obs_configure(const FlDev &d, ObsArgs &P, ObsOptions &accepted, const int *h_R) {
    if (!obs_pick_config(d, P, accepted)) return -1;
    const int n_split = h_R ? obs_take_split_class(d, P, h_R) : 0;
    if (P.tw_t == 0 && !P.merged && !P.fix) P.compact_t = 0;    // (the builder alone on the stand-alone kernel: its own pass A, teams of 32 lanes)
    return P.split ? n_split : P.fix ? d.B : 0;
}

// ---- the three launches, each in two halves: the PLAN (obs_begin, the launch's own limits and arguments, obs_configure -- host decisions
// only, what the diagnostic fl_obs_plan shares with the real launch) and obs_enqueue (output pointers, row masks, env order, the kernel)
struct ObsPlan {
    ObsArgs P;
    ObsOptions accepted;   // the options the preference walk accepted (the record's words 7 .. 20)
    int n_fit;             // envs on a launch class's body (obs_configure)
};
// voids the record (MODE -1: nothing ran -- what every failing return leaves) and checks the limits every launch has
static bool obs_begin(const FlObsScratch &o, const FlDev &d, int pred_depth, int record[FL_OBS_LAUNCH_WORDS]) {
    memset(record, 0, FL_OBS_LAUNCH_WORDS * sizeof record[0]);
    record[0] = -1;
    return d.A <= 1024 && pred_depth + 2 <= o.pred_cap && pred_depth <= 510;
}
static int obs_plan_end(const FlDev &d, ObsPlan &pl, const int *h_R) {
    pl.accepted = ObsOptions();
    pl.n_fit = obs_configure(d, pl.P, pl.accepted, h_R);
    return pl.n_fit < 0 ? FL_ERR_ARG : FL_OK;
}
static int obs_plan_cutils(const FlObsScratch &o, const FlDev &d, int max_nodes, int pred_depth, const int16_t *label_dev, int record[FL_OBS_LAUNCH_WORDS], ObsPlan &pl) {
    if (!obs_begin(o, d, pred_depth, record) || max_nodes > FL_OBS_MAX_NODES) return FL_ERR_ARG;
    pl.P = ObsArgs();
    pl.P.label = label_dev;
    obs_cutils_args(pl.P, max_nodes, pred_depth, obs_batch_is_wide(d.B, o.n_cu));
    obs_alone_args(d, pl.P);
    return obs_plan_end(d, pl, pl.P.label ? nullptr : o.h_R);   // (a handle subset: no split class)
}
static int obs_plan_both(const FlObsScratch &o, const FlDev &d, int max_nodes, int pred_depth, int max_depth, int tree_pred, double *tree_out,
                         int record[FL_OBS_LAUNCH_WORDS], ObsPlan &pl) {
    if (!obs_begin(o, d, pred_depth, record) || max_nodes > OBS_CAP_C) return FL_ERR_ARG;   // (the fused kernels: 32-lane teams)
    if (max_depth > 3 || tree_pred > pred_depth || tree_pred < 0) return FL_ERR_ARG;  // the upstream path must be a prefix
    pl.P = ObsArgs();
    obs_cutils_args(pl.P, max_nodes, pred_depth, obs_batch_is_wide(d.B, o.n_cu));
    obs_tree_args(d, pl.P, max_depth, tree_pred, tree_out);
    pl.P.keep_mode = o.keep_rows;
    pl.P.h_R = o.h_R;
    return obs_plan_end(d, pl, o.h_R);
}
static int obs_plan_tree(const FlObsScratch &o, const FlDev &d, int max_depth, int pred_depth, double *out, const int16_t *label_dev,
                         int record[FL_OBS_LAUNCH_WORDS], ObsPlan &pl) {
    if (!obs_begin(o, d, pred_depth, record) || max_depth > FL_MAX_TREE_DEPTH) return FL_ERR_ARG;
    // depth 4: compact node tables only (level L of the tree has at most 2^L nodes when no direction of a cell has more than two
    // transitions -- every Flatland rail cell type): 30 slots; the DFS-slot tables of other grids stop at depth 3 (85 slots)
    if (max_depth > 3 && d.max_branch > 2) return FL_ERR_ARG;
    pl.P = ObsArgs();
    pl.P.label = label_dev;
    obs_tree_args(d, pl.P, max_depth, pred_depth, out);
    if (max_depth > 3 && !pl.P.compact_t) return FL_ERR_ARG;   // (FL_OBS_NO_COMPACT)
    return obs_plan_end(d, pl, nullptr);   // (no split class has the upstream builder alone)
}
static int obs_enqueue(FlObsScratch &o, const FlDev &d, ObsPlan &pl, hipStream_t s, int record[FL_OBS_LAUNCH_WORDS]) {
    ObsArgs &P = pl.P;
    o.last_fix = P.fix; o.last_split = P.split; o.last_fit = pl.n_fit;
    // FL_OBS_KEEP_TREE_ROWS: the row masks of the previous launch describe this very buffer at this depth -> no pre-fill of the slab
    uint4 *const rowmask = o.rowmask;
    struct Restore { FlObsScratch &o; uint4 *m; ~Restore() { o.rowmask = m; } } restore{o, rowmask};
    if (P.tw_t) {
        P.keep_rows = o.keep_rows && o.rows_out == P.tree_out && o.rows_depth == P.max_depth;
        o.rows_out = P.tree_out; o.rows_depth = P.max_depth;
        // mode off, or more rows than the masks' 96 bits (the tree launch alone goes beyond depth 3): the kernels keep no row masks (restored on return -- `u` is a copy of o)
        if (!o.keep_rows || P.max_depth > 3) { o.rowmask = nullptr; P.keep_rows = 0; o.rows_out = nullptr; }
    }
    P.no_cf_dirs = obs_switches().no_cf_dirs; P.pb_ceil_split = obs_switches().pb_ceil_split; P.no_early_topo = obs_switches().no_early_topo;   // (what the kernels see of the switches)
    obs_verbose(P);
    obs_keep_verify(d, P, rowmask, s);
    FlObsScratch u = o;
    if (P.merged == 1) u.order = nullptr;   // small envs, one round: workgroup k builds env k
    else u = fl_obs_env_order(o, d, s);
    const int rc = obs_launch(d, u, P, s);
    if (rc == FL_OK) obs_record_launch(P, pl.accepted, record);
    return rc;
}

int fl_launch_obs_cutils(FlObsScratch &o, const FlDev &d, int max_nodes, int pred_depth, const FlObsCutilsOut &out, hipStream_t s,
                         int record[FL_OBS_LAUNCH_WORDS], const int16_t *label_dev, int out64) {
    ObsPlan pl;
    const int rc = obs_plan_cutils(o, d, max_nodes, pred_depth, label_dev, record, pl);
    if (rc != FL_OK) return rc;
    pl.P.out64 = out64;
    obs_out_args(pl.P, o, out);
    return obs_enqueue(o, d, pl, s, record);
}

int fl_launch_obs_both(FlObsScratch &o, const FlDev &d, int max_nodes, int pred_depth, const FlObsCutilsOut &out, int max_depth, int tree_pred,
                       double *tree_out, hipStream_t s, int record[FL_OBS_LAUNCH_WORDS]) {
    ObsPlan pl;
    const int rc = obs_plan_both(o, d, max_nodes, pred_depth, max_depth, tree_pred, tree_out, record, pl);
    if (rc != FL_OK) return rc;
    obs_out_args(pl.P, o, out);
    return obs_enqueue(o, d, pl, s, record);
}

int fl_launch_obs_tree(FlObsScratch &o, const FlDev &d, int max_depth, int pred_depth, double *out, hipStream_t s, int record[FL_OBS_LAUNCH_WORDS],
                       const int16_t *label_dev) {
    ObsPlan pl;
    const int rc = obs_plan_tree(o, d, max_depth, pred_depth, out, label_dev, record, pl);
    if (rc != FL_OK) return rc;
    pl.P.dbg = o.dbg;
    return obs_enqueue(o, d, pl, s, record);
}

// diagnostic, no GPU needed: the plan half of the launch `kind` (0 fl_launch_obs_cutils, 1 _both, 2 _tree: each takes of the parameters what its
// launch takes -- the tree launch's predictor depth is tree_pred) and the record that launch would leave; o: n_cu, h_R, keep_rows and pred_cap
// as the handle has them.  *n_fit: envs on a launch class's body.  FL_ERR_ARG (record voided) where the launch returns it.
int fl_obs_plan(int kind, const FlObsScratch &o, const FlDev &d, int max_nodes, int pred_depth, int max_depth, int tree_pred, const int16_t *label,
                int record[FL_OBS_LAUNCH_WORDS], int *n_fit) {
    ObsPlan pl;
    const int rc = kind == 0 ? obs_plan_cutils(o, d, max_nodes, pred_depth, label, record, pl)
                 : kind == 1 ? obs_plan_both(o, d, max_nodes, pred_depth, max_depth, tree_pred, nullptr, record, pl)
                 : kind == 2 ? obs_plan_tree(o, d, max_depth, tree_pred, nullptr, label, record, pl) : FL_ERR_ARG;
    if (rc != FL_OK) return rc;
    obs_record_launch(pl.P, pl.accepted, record);
    *n_fit = pl.n_fit;
    return FL_OK;
}

// diagnostic: the configuration obs_pick_config chooses for the fused launch (cutils + upstream tree of max_depth):
// threads, LDS bytes, static tables in LDS, next-hop in LDS, work-list bytes, time masks, second index, items in LDS
int fl_obs_config_of_fused(const FlDev &d, int pred_depth, int max_depth, int tree_pred, int out[11], int wide) {
    ObsArgs P = {};
    obs_cutils_args(P, 31, pred_depth, wide);   // (the solution's tree size; the fixed launch classes are for exactly that)
    if (max_depth > 0) obs_tree_args(d, P, max_depth, tree_pred, nullptr);
    else obs_alone_args(d, P);   // max_depth 0: the flatland_cutils builder alone (fl_launch_obs_cutils)
    ObsOptions q = {};
    if (obs_configure(d, P, q, nullptr) < 0) return FL_ERR_ARG;
    if (obs_switches().verbose) {   // diagnostic: the carving of the LDS, array by array (enum L_* of fl_obs_layout.h)
        fprintf(stderr, "  options {nt %d, wl_bytes %d, tab %d, nh %d, tmask %d, dual %d, items %d, snext %d, partial %d, bk_room %d, own_filter %d, fb %d, raw %d, items_cap %d, wl_head %d}; "
                        "shape {merged %d, tw_c %d, tw_t %d, tpw_t %d, tree_pred %d}; bk %d tshift %d wl_occ_div %d\n",
                q.nt, q.wl_bytes, q.tab, q.nh, q.tmask, q.dual, q.items, q.snext, q.partial, q.bk_room, q.own_filter, q.fb, q.raw, q.items_cap, q.wl_head,
                P.merged, P.tw_c, P.tw_t, P.tpw_t, P.tree_pred, P.bk, P.tshift, P.wl_occ_div);
        static const char *names[L_COUNT] = {"cellw", "nbr", "snext", "rkey", "slot_agent", "slot_ready", "cell_target", "a_speed", "a_vpos", "a_pos", "a_tslot",
            "a_target", "a_malf", "a_tpc", "a_tq", "a_tq2", "a_raw", "rtype", "a_lp", "a_n", "a_srank", "a_dir", "a_state", "a_free", "a_dead", "misc", "team_meta", "node_tables",
            "csr", "items", "wl", "partial", "tmask", "tmask2", "nh", "csr2", "tmaskb", "tmaskb2", "items2", "a_lp2", "a_tpc2", "bkrel", "seg", "dm", "hop8", "cmask", "cmaskb"};
        for (int k = 0; k < L_COUNT; k++) {
            if (P.L.off[k] == L_ABSENT) continue;
            unsigned next = P.L.total;
            for (int j = 0; j < L_COUNT; j++) if (P.L.off[j] != L_ABSENT && P.L.off[j] > P.L.off[k] && P.L.off[j] < next) next = P.L.off[j];
            fprintf(stderr, "  %-12s %7u B\n", names[k], next - P.L.off[k]);
        }
    }
    out[0] = P.L.nt; out[1] = (int)P.L.total; out[2] = P.L.tab_lds; out[3] = P.L.off[L_NH] != L_ABSENT; out[4] = P.L.wl_bytes;
    out[5] = P.use_tmask + 2 * (P.L.off[L_TMASK2] != L_ABSENT);                    // 3: time masks + the own-path filter's second set
    out[6] = P.dual_index; out[7] = P.L.off[L_ITEMS] != L_ABSENT ? P.L.items_cap : 0;  // entries of the LDS copy of the items
    out[8] = P.merged; out[9] = P.compact_t; out[10] = P.fix;   // fixed launch class (compile-time LDS carving), 0 = none
    return FL_OK;
}
