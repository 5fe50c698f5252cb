// fl_static.h -- the host-only static description of a batch's envs: what fl_load_env stages, the rail-cell index space fl_commit
// derives from it, and the owner election of the shared static tables (FlDev::tab).  Nothing here calls the HIP API: fl_host.hip
// does the device half (allocation, upload, the table kernels), and the fl_debug_static_* hooks run this half alone, without a GPU.
//
// fl_static_arrays is the ONE list of the arrays that exist both here and on the device.  A new static table is one line in it
// plus its FlDev pointer.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/flatland_hip.h"
#include "fl_internal.h"

struct FlStatic {
    int B = 0, A = 0, H = 0, W = 0;
    int Ucap = 0, Rcap = 0;            // capacity per env (unique targets, rail cells), fixed at the first commit
    int reserve_U = 0, reserve_R = 0;  // fl_reserve: capacity for envs loaded after the first commit
    bool committed = false;
    // every env's static description (filled by fl_load_env; kept after commit: live map replacement, fl_distance_map's expansion
    // to the dense layout).  The arrays of fl_static_arrays carry their device copy's name.
    std::vector<uint32_t> gridx;  // the device's copy of the grid: transitions | neighbour-has-rail bits (FlDev::grid)
    std::vector<uint16_t> grid, ridx, rgrid, nbr, rkey, init_r, target_r, ut_r, srank;
    std::vector<int> maxbr;       // per env: most transitions of any (cell, direction)
    std::vector<uint32_t> rcell;  // cell id of a rail index (fl_predict turns waypoints back into cells)
    std::vector<int> init_pos, target, earliest, latest, tslot, ut, U, R, K, T, mt_pos, malf_min, malf_max;
    std::vector<uint32_t> spk, mt;
    std::vector<double> speed;
    std::vector<uint64_t> malf_thr;
    std::vector<uint8_t> loaded, dirty;  // dirty: loaded since the last commit
    std::vector<uint8_t> rtype;
    // shared static tables: key = content id of env b's map side (rail grid + unique targets), tab = the owner of its tables,
    // built = content id of what env b's slabs hold on the device (0 = nothing yet), need = the owners a commit (re)builds
    std::vector<uint64_t> key, built;
    std::vector<int> tab;
    std::vector<uint8_t> need;
};

// Every array that exists on the host (FlStatic) and on the device (FlDev, and rcell_dev beside it), with its elements per env --
// stated here and nowhere else -- and the value a never-loaded env holds on the host.  visit(name, host vector, device pointer,
// elements per env, fill, present) returns FL_OK or ends the walk with its code.  present: rkey exists only on maps taller than wide.
template <class V>
static inline int fl_static_arrays(FlStatic &s, FlDev &d, uint32_t *&rcell_dev, V &&visit) {
    const size_t A = (size_t)s.A, HW = (size_t)s.H * s.W, R = (size_t)s.Rcap, U = (size_t)s.Ucap;
    int rc = FL_OK;
    auto v = [&](const char *name, auto &host, auto *&dev, size_t per_env, int fill = 0, bool present = true) {
        if (rc == FL_OK) rc = visit(name, host, dev, per_env, fill, present);
    };
    v("T", s.T, d.T, 1); v("mt_pos", s.mt_pos, d.mt_pos, 1, 624); v("mt", s.mt, d.mt, 624);   // per env
    v("malf_thr", s.malf_thr, d.malf_thr, 1); v("malf_min", s.malf_min, d.malf_min, 1); v("malf_max", s.malf_max, d.malf_max, 1);
    v("U", s.U, d.U, 1); v("R", s.R, d.R, 1); v("K", s.K, d.K, 1);
    v("gridx", s.gridx, d.grid, HW); v("ridx", s.ridx, d.ridx, HW, FL_R_NONE);   // per cell
    v("rgrid", s.rgrid, d.rgrid, R); v("rtype", s.rtype, d.rtype, R); v("nbr", s.nbr, d.nbr, R * 4, FL_R_NONE);   // per rail cell
    v("rkey", s.rkey, d.rkey, R, 0, s.H > s.W); v("rcell", s.rcell, rcell_dev, R); v("ut_r", s.ut_r, d.ut_r, U);   // (ut_r: per unique target)
    v("init_pos", s.init_pos, d.init_pos, A); v("target", s.target, d.target, A); v("init_r", s.init_r, d.init_r, A); v("target_r", s.target_r, d.target_r, A); v("srank", s.srank, d.srank, A);   // per agent
    v("earliest", s.earliest, d.earliest, A); v("latest", s.latest, d.latest, A); v("tslot", s.tslot, d.tslot, A); v("spk", s.spk, d.spk, A); v("speed", s.speed, d.speed, A, 1);
    return rc;
}

// the host side of the list alone: visit(name, host vector, elements per env, fill, present)
template <class V>
static inline void fl_static_host_arrays(FlStatic &s, V &&visit) {
    FlDev none = {};
    uint32_t *none_rcell = nullptr;
    fl_static_arrays(s, none, none_rcell, [&](const char *name, auto &host, auto *&, size_t per_env, int fill, bool present) {
        visit(name, host, per_env, fill, present);
        return (int)FL_OK;
    });
}
// size every listed array that is empty (an absent one stays empty)
static inline void fl_static_size_arrays(FlStatic &s) {
    fl_static_host_arrays(s, [&](const char *, auto &host, size_t per_env, int fill, bool present) {
        if (host.empty() && present) host.assign((size_t)s.B * per_env, (typename std::decay_t<decltype(host)>::value_type)fill);
    });
}

// a batch of B envs of A agents on H x W maps, nothing loaded (fl_create's size checks)
static inline int fl_static_init(FlStatic &s, int B, int A, int H, int W) {
    if (B <= 0 || A <= 0 || H <= 0 || W <= 0) { fl_set_error("fl_create: bad sizes"); return FL_ERR_ARG; }
    if (A > 1024) { fl_set_error("fl_create: at most 1024 agents per env (one lane per agent), got %d", A); return FL_ERR_ARG; }
    if ((long long)H * W * 4 >= (1ll << 30)) { fl_set_error("fl_create: map too large"); return FL_ERR_ARG; }
    s = FlStatic();
    s.B = B; s.A = A; s.H = H; s.W = W;
    fl_static_size_arrays(s);   // (capacities 0: the arrays sized by them stay empty until the first commit)
    s.grid.assign((size_t)B * H * W, 0); s.ut.assign((size_t)B * A, 0); s.maxbr.assign(B, 0);
    s.loaded.assign(B, 0); s.dirty.assign(B, 0);
    s.key.assign(B, 0); s.built.assign(B, 0); s.tab.assign(B, 0); s.need.assign(B, 0);
    return FL_OK;
}

// fl_reserve; fits(max_rail_cells): the device side's own limit (it sets the message of its refusal)
template <class Fits>
static inline int fl_static_reserve(FlStatic &s, int max_targets, int max_rail_cells, Fits &&fits) {
    if (max_targets < 0 || max_rail_cells < 0) { fl_set_error("fl_reserve: bad argument"); return FL_ERR_ARG; }
    if (s.committed) { fl_set_error("fl_reserve: the capacities are fixed at the first fl_commit"); return FL_ERR_ARG; }
    if ((long long)max_rail_cells * 4 > 65532) { fl_set_error("fl_reserve: at most 16383 rail cells per env (u16 rail states)"); return FL_ERR_ARG; }
    if (!fits(max_rail_cells)) return FL_ERR_ARG;
    s.reserve_U = max_targets > s.A ? s.A : max_targets;
    s.reserve_R = max_rail_cells;
    return FL_OK;
}

// fl_load_env after the handle check: stage env b
static inline int fl_static_load(FlStatic &s, int b, const uint16_t *grid, const int32_t *init_pos, const int32_t *init_dir,
                                 const int32_t *target, const double *speed, const int32_t *earliest, const int32_t *latest,
                                 int max_episode_steps, uint64_t malf_threshold, int malf_min, int malf_max, const uint32_t *mt_key,
                                 int mt_pos) {
    if (b < 0 || b >= s.B) { fl_set_error("fl_load_env: env index out of range"); return FL_ERR_ARG; }
    if (!grid || !init_pos || !init_dir || !target || !speed || !earliest || !latest || !mt_key) { fl_set_error("fl_load_env: null argument"); return FL_ERR_ARG; }
    const int A = s.A, H = s.H, W = s.W;
    const size_t HW = (size_t)H * W;
    if (mt_pos < 0 || mt_pos > 624) { fl_set_error("fl_load_env: mt_pos out of range"); return FL_ERR_ARG; }
    if (malf_max < malf_min || malf_min < 0 || malf_max > 60000) { fl_set_error("fl_load_env: bad malfunction duration range"); return FL_ERR_ARG; }
    size_t rail_cells = 0;
    for (size_t c = 0; c < HW; c++) rail_cells += grid[c] != 0;
    if (rail_cells * 4 > 65532) { fl_set_error("fl_load_env: %zu rail cells exceed the u16 rail-state / distance range", rail_cells); return FL_ERR_ARG; }
    // validate everything before touching the staged copy of env b (a refused call leaves it as it was)
    std::vector<int> ut;
    std::vector<int> tslot(A);
    for (int i = 0; i < A; i++) {
        const int ir = init_pos[2 * i], ic = init_pos[2 * i + 1], tr = target[2 * i], tc = target[2 * i + 1];
        if (ir < 0 || ir >= H || ic < 0 || ic >= W || tr < 0 || tr >= H || tc < 0 || tc >= W || init_dir[i] < 0 || init_dir[i] > 3) {
            fl_set_error("fl_load_env: agent %d position/direction out of range", i);
            return FL_ERR_ARG;
        }
        if (grid[(size_t)ir * W + ic] == 0 || grid[(size_t)tr * W + tc] == 0) { fl_set_error("fl_load_env: agent %d starts or ends on a cell without rail", i); return FL_ERR_ARG; }
        if (!(speed[i] > 0.0) || speed[i] > 1.0) { fl_set_error("fl_load_env: agent %d speed %g not in (0, 1]", i, speed[i]); return FL_ERR_ARG; }
        const int max_count = (int)(1.0 / speed[i]) - 1;  // SpeedCounter.max_count (step_utils/speed_counter.py:39-41)
        if (max_count < 0 || max_count > FL_MAX_SPEED_COUNT) { fl_set_error("fl_load_env: agent %d speed %g unsupported (max_count %d)", i, speed[i], max_count); return FL_ERR_ARG; }
        // unique targets in first-seen order (distance_map.py:71-79)
        const int tcell = tr * W + tc;
        size_t u = 0;
        for (; u < ut.size(); u++)
            if (ut[u] == tcell) break;
        if (u == ut.size()) ut.push_back(tcell);
        tslot[i] = (int)u;
    }
    if (s.committed && ((int)ut.size() > s.Ucap || (int)rail_cells > s.Rcap)) {
        fl_set_error("fl_load_env: env %d has %zu unique targets / %zu rail cells, the batch was committed for %d / %d (fl_reserve)", b,
                     ut.size(), rail_cells, s.Ucap, s.Rcap);
        return FL_ERR_CAPACITY;
    }
    {   // another map or other unique targets than the staged ones: whatever env b's slabs hold is stale, whatever its content key says
        bool same = s.loaded[b] && s.U[b] == (int)ut.size() && memcmp(&s.grid[b * HW], grid, HW * 2) == 0;
        for (size_t u = 0; same && u < ut.size(); u++) same = s.ut[(size_t)b * A + u] == ut[u];
        if (!same) s.built[b] = 0;
    }
    memcpy(&s.grid[b * HW], grid, HW * 2);
    for (int i = 0; i < A; i++) {
        const size_t g = (size_t)b * A + i;
        s.init_pos[g] = init_pos[2 * i] * W + init_pos[2 * i + 1];
        s.target[g] = target[2 * i] * W + target[2 * i + 1];
        s.earliest[g] = earliest[i];
        s.latest[g] = latest[i];
        s.speed[g] = speed[i];
        s.spk[g] = (uint32_t)init_dir[i] | ((uint32_t)((int)(1.0 / speed[i]) - 1) << 2);
        s.tslot[g] = tslot[i];
        s.ut[g] = i < (int)ut.size() ? ut[i] : 0;
        int rank = 0;
        for (int j = 0; j < A; j++) rank += speed[j] < speed[i];
        s.srank[g] = (uint16_t)rank;
    }
    {
        int mb = 0;
        for (size_t c = 0; c < HW; c++)
            for (int dd = 0; dd < 4; dd++) mb = std::max(mb, __builtin_popcount((grid[c] >> ((3 - dd) * 4)) & 15u));
        s.maxbr[b] = mb;
    }
    s.U[b] = (int)ut.size();
    s.R[b] = (int)rail_cells;
    s.T[b] = max_episode_steps;
    s.malf_thr[b] = malf_threshold;
    s.malf_min[b] = malf_min;
    s.malf_max[b] = malf_max;
    memcpy(&s.mt[(size_t)b * 624], mt_key, 624 * 4);
    s.mt_pos[b] = mt_pos;
    s.loaded[b] = 1;
    s.dirty[b] = 1;
    return FL_OK;
}

// most transitions any (rail cell, direction) of the batch has (FlDev::max_branch)
static inline int fl_static_max_branch(const FlStatic &s) { return *std::max_element(s.maxbr.begin(), s.maxbr.end()); }

// RailEnvTransitions.transition_list (core/grid/rail_env_grid.py:28-38)
static const uint16_t k_transition_list[11] = {0x0000, 0x8020, 0x9220, 0x8421, 0x9621, 0xCC33, 0x5202, 0x2000, 0x4002, 0x1200, 0xC022};
// rotate_transition (flatland_cutils/src/tool.h:300-335): each nibble rotated right by k, then the word by 4k
static inline uint32_t rotate_transition(uint32_t cell, int k) {
    uint32_t v = 0;
    for (int i = 0; i < 4; i++) {
        uint32_t nib = (cell >> ((3 - i) * 4)) & 15u;
        nib = ((nib >> k) | (nib << (4 - k))) & 15u;
        v |= nib << ((3 - i) * 4);
    }
    return ((v >> (4 * k)) | (v << (16 - 4 * k))) & 0xFFFFu;
}
// road_type of a cell (flatland_cutils/src/loader.cpp:122-161): the first basic transition one of its four rotations equals
static inline int road_type_of(uint32_t cell) {
    for (int rot = 0; rot < 4; rot++) {
        const uint32_t t = rot == 0 ? cell : rotate_transition(cell, rot);
        for (int k = 0; k < 11; k++)
            if (k_transition_list[k] == t) return k;
    }
    return 0;
}

// rail-cell index space of env b (fl_internal.h): ridx / rcell / rgrid / nbr / rkey, the agents' and targets' rail indices
static inline void build_rail_tables(FlStatic &s, int b) {
    const int A = s.A, H = s.H, W = s.W, Rcap = s.Rcap, Ucap = s.Ucap;
    const size_t HW = (size_t)H * W;
    const uint16_t *grid = &s.grid[b * HW];
    uint16_t *ridx = &s.ridx[b * HW];
    uint32_t *rcell = &s.rcell[(size_t)b * Rcap];
    uint16_t *rgrid = &s.rgrid[(size_t)b * Rcap], *nbr = &s.nbr[(size_t)b * Rcap * 4];
    int R = 0;
    for (size_t c = 0; c < HW; c++) {
        if (grid[c]) { ridx[c] = (uint16_t)R; rcell[R] = (uint32_t)c; rgrid[R] = grid[c]; s.rtype[(size_t)b * Rcap + R] = (uint8_t)road_type_of(grid[c]); R++; }
        else ridx[c] = FL_R_NONE;
    }
    for (int r = R; r < Rcap; r++) { rcell[r] = 0; rgrid[r] = 0; }
    // the step kernel's copy of the grid: one load answers "which transitions" and "does the cell towards m have rail"
    // (check_valid_action, transition_utils.py:47-82)
    uint32_t *gridx = &s.gridx[b * HW];
    for (size_t c = 0; c < HW; c++) {
        const int row = (int)(c / W), col = (int)(c % W);
        uint32_t v = grid[c];
        for (int m = 0; m < 4; m++) {
            const int nr = row + (m == 0 ? -1 : m == 2 ? 1 : 0), nc = col + (m == 1 ? 1 : m == 3 ? -1 : 0);
            if (nr >= 0 && nr < H && nc >= 0 && nc < W && grid[(size_t)nr * W + nc] != 0) v |= 1u << (16 + m);
        }
        gridx[c] = v;
    }
    for (int r = 0; r < Rcap; r++) {
        const int row = r < R ? (int)(rcell[r] / W) : 0, col = r < R ? (int)(rcell[r] % W) : 0;
        for (int m = 0; m < 4; m++) {
            const int nr = row + (m == 0 ? -1 : m == 2 ? 1 : 0), nc = col + (m == 1 ? 1 : m == 3 ? -1 : 0);
            nbr[r * 4 + m] = (r < R && nr >= 0 && nr < H && nc >= 0 && nc < W) ? ridx[(size_t)nr * W + nc] : FL_R_NONE;
        }
    }
    int K = R;
    if (H > W) {  // flatland_cutils keys its prediction maps by col * W + row (tool.h:391-398), which collides on tall maps:
                  // rail cells with equal keys share one compact key
        std::vector<uint32_t> keys(R);
        for (int r = 0; r < R; r++) keys[r] = (rcell[r] % W) * (uint32_t)W + rcell[r] / W;
        std::vector<uint32_t> uniq(keys);
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        K = (int)uniq.size();
        uint16_t *rkey = &s.rkey[(size_t)b * Rcap];
        for (int r = 0; r < R; r++) rkey[r] = (uint16_t)(std::lower_bound(uniq.begin(), uniq.end(), keys[r]) - uniq.begin());
        for (int r = R; r < Rcap; r++) rkey[r] = 0;
    }
    s.K[b] = K;
    for (int i = 0; i < A; i++) {
        const size_t g = (size_t)b * A + i;
        s.init_r[g] = ridx[s.init_pos[g]];
        s.target_r[g] = ridx[s.target[g]];
    }
    for (int u = 0; u < Ucap; u++) s.ut_r[(size_t)b * Ucap + u] = u < s.U[b] ? ridx[s.ut[(size_t)b * A + u]] : 0;
}

// content id of env b's map side: FNV-1a over the rail grid and the unique targets (what the static tables are a function of)
static inline uint64_t map_content_key(const FlStatic &s, int b) {
    const size_t HW = (size_t)s.H * s.W;
    uint64_t k = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) {
        const unsigned char *c = (const unsigned char *)p;
        for (size_t i = 0; i < n; i++) { k ^= c[i]; k *= 1099511628211ull; }
    };
    mix(&s.grid[b * HW], HW * 2);
    const int U = s.U[b];
    mix(&U, sizeof U);
    mix(&s.ut[(size_t)b * s.A], (size_t)U * sizeof(int));
    return k ? k : 1;
}
static inline bool same_map_content(const FlStatic &s, int a, int b) {
    const size_t HW = (size_t)s.H * s.W;
    return s.U[a] == s.U[b] && memcmp(&s.grid[a * HW], &s.grid[b * HW], HW * 2) == 0 &&
           memcmp(&s.ut[(size_t)a * s.A], &s.ut[(size_t)b * s.A], (size_t)s.U[a] * sizeof(int)) == 0;
}
// owners of the static tables (tab -> FlDev::tab) and the owners whose slabs have to be (re)built (need -> fl_batch::need_dev)
static inline void elect_table_owners(FlStatic &s) {
    static const bool no_share = getenv("FL_NO_SHARED_TABLES") != nullptr;   // diagnostic: every env reads its own slabs
    const int B = s.B;
    for (int b = 0; b < B; b++)
        if (s.dirty[b]) s.key[b] = map_content_key(s, b);
    std::vector<std::pair<uint64_t, int>> order(B);
    for (int b = 0; b < B; b++) order[b] = {s.key[b], b};
    std::sort(order.begin(), order.end());
    for (int i = 0; i < B;) {
        int j = i;
        while (j < B && order[j].first == order[i].first) j++;
        // envs of one key, ascending: the first env with identical content is the owner (a hash collision keeps its own tables)
        for (int k = i; k < j; k++) {
            const int b = order[k].second;
            int owner = b;
            if (!no_share)
                for (int q = i; q < k; q++)
                    if (s.tab[order[q].second] == order[q].second && same_map_content(s, order[q].second, b)) { owner = order[q].second; break; }
            s.tab[b] = owner;
        }
        i = j;
    }
    // (built is set by fl_static_commit_end once the table kernels of the need envs have run: a commit that fails half way rebuilds them)
    for (int b = 0; b < B; b++) s.need[b] = s.tab[b] == b && s.built[b] != s.key[b];
}

// The host half of fl_commit before the device work.  The first commit fixes the capacities and sizes the arrays that depend on them;
// every commit (re)builds the host tables of the envs loaded since the last one and elects the owners of the shared tables.
// *any: an env was loaded since the last commit (otherwise there is nothing to upload or build).
static inline int fl_static_commit_begin(FlStatic &s, bool *any) {
    for (int b = 0; b < s.B; b++)
        if (!s.loaded[b]) { fl_set_error("fl_commit: env %d was never loaded", b); return FL_ERR_ARG; }
    if (!s.committed) {
        // (a first commit that failed on the device side comes here again: the arrays sized by the capacities start over)
        s.Ucap = s.Rcap = 0;
        fl_static_host_arrays(s, [](const char *, auto &host, size_t per_env, int, bool) { if (per_env == 0) host.clear(); });
        s.Ucap = s.reserve_U > 1 ? s.reserve_U : 1;
        s.Rcap = s.reserve_R > 1 ? s.reserve_R : 1;
        for (int b = 0; b < s.B; b++) {
            s.Ucap = std::max(s.Ucap, s.U[b]);
            s.Rcap = std::max(s.Rcap, s.R[b]);
        }
        fl_static_size_arrays(s);
    }
    *any = false;
    for (int b = 0; b < s.B; b++) {
        if (!s.dirty[b]) continue;
        *any = true;
        build_rail_tables(s, b);
    }
    if (*any) elect_table_owners(s);
    return FL_OK;
}
// ... and after it: the owners' slabs hold their content now, nothing is dirty
static inline void fl_static_commit_end(FlStatic &s) {
    for (int b = 0; b < s.B; b++)
        if (s.need[b]) s.built[b] = s.key[b];
    std::fill(s.dirty.begin(), s.dirty.end(), 0);
    s.committed = true;
}
