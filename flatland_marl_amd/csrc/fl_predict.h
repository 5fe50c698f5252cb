// fl_predict.h -- flatland.envs.predictions.ShortestPathPredictorForRailEnv.get() (predictions.py:97-180) on top of
// get_shortest_paths(distance_map, max_depth) (rail_env_shortest_paths.py:203-274) for a range of envs, one launch (gfx950).
// Included by fl_host.hip, next to its entry point fl_predict (include/flatland_predict.h).
//
// Per agent the reference returns
//   the path    the waypoints (row, col, dir) of the strict greedy descent of the distance map from the agent's start -- initial_position
//               off the map, position on it, target when DONE, always with agent.direction -- until the target cell, cut after max_depth
//               waypoints (a cut path has exactly max_depth of them); None when a step finds nothing closer
//   get()       float64 [max_depth + 1][5] rows (time, row, col, dir, action): with tpc = int(1 / speed), m = len(path) - 1 (0 for
//               None) row i stands on waypoint min(i / tpc, m), and its action is STOP_MOVING (4) when row i - 1 already stood on
//               waypoint m -- (i - 1) / tpc >= m -- else 0.  (The reference's loop takes a new waypoint at i % tpc == 0 while it has
//               one left and is not on the target, and a path only ends on the target or at the cut: the closed form is that loop.)
// The descent is static per (target, rail cell, orientation): FlDev::nh holds its next hop and FlDev::hop8 the state eight hops on,
// FL_R_NONE when the path ends earlier -- on the target, where nothing is closer, or where the rail is disconnected.
//
// Kernel: one workgroup of FLP_THREADS lanes per `ga` consecutive agents of the range's [nb][A] order (ga <= FLP_THREADS / 8).
//   1. EIGHT lanes walk one agent's path as k_obs does: lane j takes j single hops through nh, then eight hops at a time through
//      hop8, and records the rail states of the waypoints j, j + 8, ... in LDS.  The path's length is the highest index recorded
//      + 1; a path that does not end on the target is None unless it was cut, and a cut path is None when its last waypoint has no
//      next hop (the reference looks for one before it counts the waypoint).
//   2. every lane expands rows: row i of an agent -> (row, col << 3 | dir << 1 | stop) in LDS, the cell of a rail index from `rcell`
//   3. every lane streams: the agents' blocks are one contiguous run of the output, written as aligned 16-byte words (scalar stores
//      where a block starts or ends inside a word), each element picked from the LDS rows; the waypoints as 4-byte stores.
// Reads: 36 B of agent rows and a chain of at most 7 + max_depth / 8 dependent table gathers per agent; writes: everything.
// Every loop is bounded by max_depth, every table index comes from a table or is checked, nothing is written outside the outputs.
#pragma once
#include "fl_internal.h"

#ifndef FLP_THREADS
#define FLP_THREADS 256
#endif
#ifndef FLP_LDS_BUDGET
#define FLP_LDS_BUDGET (32 * 1024)   // bytes a workgroup
#endif
#ifndef FLP_WG_PER_CU
#define FLP_WG_PER_CU 2              // agents a workgroup are halved (down to 4) until the grid has this many workgroups a CU
#endif
#define FLP_MAX_DEPTH 500

template <typename T> struct flp_vec;
template <> struct flp_vec<int32_t> { typedef int32_t type __attribute__((ext_vector_type(4))); };
template <> struct flp_vec<double> { typedef double type __attribute__((ext_vector_type(2))); };

// LDS per agent slot: rows int2[D + 1], then the path u16[D] padded to 8 bytes
__host__ __device__ static inline size_t flp_slot_bytes(int D) { return (size_t)(D + 1) * 8 + (((size_t)D * 2 + 7) & ~(size_t)7); }
static inline size_t flp_lds_bytes(int ga, int D) { return (size_t)ga * flp_slot_bytes(D); }

// grid (ceil(nb * A / ga)); dynamic LDS = flp_lds_bytes(ga, D).  pred: [nb][A][D + 1][5] or nullptr; path [nb][A][D][3] and
// path_len [nb][A], both or neither.  rcell: [B][Rcap] cell id of a rail index.
template <typename T>
__global__ void __launch_bounds__(FLP_THREADS) k_predict(FlDev d, const uint32_t *__restrict__ rcell, int b0, int nb, int D, int ga,
                                                         T *__restrict__ pred, int32_t *__restrict__ path_out,
                                                         int32_t *__restrict__ path_len) {
    extern __shared__ __align__(16) unsigned char flp_lds[];
    __shared__ int s_n[FLP_THREADS / 8];       // waypoints of the path (0 = None)
    __shared__ int s_cell0[FLP_THREADS / 8];   // the start: cell id
    __shared__ int s_dir0[FLP_THREADS / 8];    //            direction
    __shared__ int s_tpc[FLP_THREADS / 8];     // times_per_cell
    __shared__ int s_tb[FLP_THREADS / 8];      // the env that holds the agent's static tables
    const int A = d.A, W = d.W, HW = d.H * d.W, Rcap = d.Rcap, Scap = d.Rcap * 4;
    const int tid = threadIdx.x;
    const long long total = (long long)nb * A;
    const long long q0 = (long long)blockIdx.x * ga;             // first agent of the workgroup in the range's order
    const int na = (int)min((long long)ga, total - q0);
    if (na <= 0) return;
    const size_t slot_bytes = flp_slot_bytes(D);
    auto rows_of = [&](int slot) { return reinterpret_cast<int2 *>(flp_lds + (size_t)slot * slot_bytes); };
    auto path_of = [&](int slot) { return reinterpret_cast<uint16_t *>(flp_lds + (size_t)slot * slot_bytes + (size_t)(D + 1) * 8); };

    // ---- 1. the walk: eight lanes an agent
    {
        const int slot = tid >> 3, j = tid & 7;
        const bool have = slot < na;
        const size_t g = (size_t)b0 * A + (size_t)(q0 + (have ? slot : 0));
        const int b = (int)(g / A), tb = d.tab[b];
        const uint32_t pk = d.pk[g], state = PK_STATE(pk), dir0 = PK_DIR(pk);
        const int tcell = d.target[g];
        const uint32_t tr = d.target_r[g];
        int cell0;
        uint32_t r0;
        if (is_off_map(state)) { cell0 = d.init_pos[g]; r0 = d.init_r[g]; }
        else if (state == ST_DONE) { cell0 = tcell; r0 = tr; }
        else {
            cell0 = d.pos[g];
            r0 = cell0 >= 0 && cell0 < HW ? (uint32_t)d.ridx[(size_t)tb * HW + cell0] : (uint32_t)FL_R_NONE;
        }
        const int u = d.tslot[g];
        const bool valid = r0 < (uint32_t)Rcap && u >= 0 && u < d.Ucap;   // (a start without rail: no path, the rows stay on it)
        const uint16_t *nh = d.nh + ((size_t)tb * d.Ucap + (valid ? u : 0)) * Rcap;
        const uint16_t *h8 = d.hop8 + ((size_t)tb * d.Ucap + (valid ? u : 0)) * Scap;
        const uint16_t *nbr = d.nbr + (size_t)tb * Scap;
        uint16_t *path = path_of(have ? slot : 0);
        uint32_t st = ((valid ? r0 : 0u) << 2) | dir0;
        bool alive = have && valid && j < D;
        // lane j: j single hops.  A hop from the target cell is never taken: the path ends there
        for (int h = 0; h < 7; h++) {
            if (alive && h < j) {
                const uint32_t hop = (st >> 2) == tr ? 4u : ((uint32_t)nh[st >> 2] >> (3u * (st & 3u))) & 7u;
                const uint32_t nr = hop >= 4u ? (uint32_t)FL_R_NONE : (uint32_t)nbr[(st & ~3u) | hop];
                if (nr >= (uint32_t)Rcap) alive = false;
                else st = (nr << 2) | hop;
            }
        }
        int idx = j, last = -1;
        for (int it = 0; it * 8 < D; it++) {       // (at most ceil(D / 8) waypoints a lane)
            if (alive) {
                path[idx] = (uint16_t)st;
                last = idx;
                const uint32_t s8 = idx + 8 < D && (st >> 2) != tr ? (uint32_t)h8[st] : (uint32_t)FL_R_NONE;
                if (s8 >= (uint32_t)Scap) alive = false;
                else { st = s8; idx += 8; }
            }
        }
        int m = last;
        m = max(m, __shfl_xor(m, 1)); m = max(m, __shfl_xor(m, 2)); m = max(m, __shfl_xor(m, 4));
        if (have && j == 0) {
            s_n[slot] = m + 1;          // (not final: step 1b)
            s_cell0[slot] = cell0;
            s_dir0[slot] = (int)dir0;
            s_tpc[slot] = (int)SPK_MAX_COUNT(d.spk[g]) + 1;   // int(1 / speed) in float64, taken on the host when the env was loaded
            s_tb[slot] = tb;
        }
    }
    __syncthreads();
    // ---- 1b. None: a path that does not stand on the target at its end and was not cut, or was cut where nothing is closer
    if ((tid & 7) == 0 && (tid >> 3) < na) {
        const int slot = tid >> 3;
        const int n = s_n[slot];
        if (n > 0) {
            const size_t g = (size_t)b0 * A + (size_t)(q0 + slot);
            const uint32_t tr = d.target_r[g];
            const uint32_t st = path_of(slot)[n - 1];
            if ((st >> 2) != tr) {
                bool none = n < D;
                if (!none) {
                    const int tb = s_tb[slot];
                    const uint16_t *nh = d.nh + ((size_t)tb * d.Ucap + d.tslot[g]) * Rcap;    // (tslot was checked: n > 0)
                    const uint32_t hop = ((uint32_t)nh[st >> 2] >> (3u * (st & 3u))) & 7u;
                    none = hop >= 4u || (uint32_t)d.nbr[(size_t)tb * Scap + ((st & ~3u) | hop)] >= (uint32_t)Rcap;
                }
                if (none) s_n[slot] = 0;
            }
        }
    }
    __syncthreads();

    // (row, col, dir) of waypoint k of an agent slot
    auto waypoint = [&](int slot, int k, int *row, int *col, int *dir) {
        int cell, dd;
        if (k == 0) { cell = s_cell0[slot]; dd = s_dir0[slot]; }
        else {
            const uint32_t st = path_of(slot)[k];
            cell = (int)rcell[(size_t)s_tb[slot] * Rcap + (st >> 2)];
            dd = (int)(st & 3u);
        }
        *row = cell / W;
        *col = cell - *row * W;
        *dir = dd;
    };

    const size_t first = (size_t)q0;     // the workgroup's first agent in the outputs
    // ---- the waypoints and their number
    if (path_out != nullptr) {
        for (int t = tid; t < na; t += FLP_THREADS) path_len[first + t] = s_n[t];
        int32_t *out = path_out + first * D * 3;
        for (int t = tid; t < na * D; t += FLP_THREADS) {
            const int slot = t / D, k = t - slot * D;
            int row = -1, col = -1, dir = -1;
            if (k < s_n[slot]) waypoint(slot, k, &row, &col, &dir);
            out[(size_t)t * 3 + 0] = row;
            out[(size_t)t * 3 + 1] = col;
            out[(size_t)t * 3 + 2] = dir;
        }
    }
    if (pred == nullptr) return;

    // ---- 2. the rows
    const int Tn = D + 1;
    for (int t = tid; t < na * Tn; t += FLP_THREADS) {
        const int slot = t / Tn, i = t - slot * Tn;
        const int tpc = s_tpc[slot], m = max(s_n[slot] - 1, 0);
        const int k = min(i / tpc, m);
        const int stop = i >= 1 && (i - 1) / tpc >= m;
        int row, col, dir;
        waypoint(slot, k, &row, &col, &dir);
        rows_of(slot)[i] = make_int2(row, (col << 3) | (dir << 1) | stop);
    }
    __syncthreads();

    // ---- 3. the stream: agent slot i owns the elements [s, s + n) of pred, one lane writes one aligned 16-byte word
    typedef typename flp_vec<T>::type VT;
    constexpr int V = 16 / sizeof(T);
    const int n = Tn * 5;
    const int mw = (n + V - 1) / V + 1;   // aligned words a run of n elements can touch
    auto value = [&](const int2 *rows, int k) {
        const int i = k / 5, c = k - i * 5;
        const int2 r = rows[i];
        const int v = c == 0 ? i : c == 1 ? r.x : c == 2 ? r.y >> 3 : c == 3 ? (r.y >> 1) & 3 : (r.y & 1) * ACT_STOP;
        return (T)v;
    };
    for (int t = tid; t < na * mw; t += FLP_THREADS) {
        const int i = t / mw, w = t - i * mw;
        const size_t s = (first + i) * (size_t)n;
        const size_t gw = s / V + w;                                 // aligned word of pred
        const long long k0 = (long long)(gw * V) - (long long)s;     // local index of its first element (< 0 at a run's head)
        if (k0 >= n) continue;
        const int2 *rows = rows_of(i);
        if (k0 >= 0 && k0 + V <= n) {
            VT v;
#pragma unroll
            for (int e = 0; e < V; e++) v[e] = value(rows, (int)k0 + e);
            *reinterpret_cast<VT *>(pred + gw * V) = v;
        } else {
#pragma unroll
            for (int e = 0; e < V; e++) {
                const long long k = k0 + e;
                if (k < 0 || k >= n) continue;
                pred[gw * V + e] = value(rows, (int)k);
            }
        }
    }
}

// agents a workgroup: what the LDS budget holds, at most one per eight lanes; halved down to 4 while the grid is small
static inline int flp_shape(long long agents, int D, int n_cu) {
    int ga = (int)std::min<size_t>(FLP_THREADS / 8, FLP_LDS_BUDGET / flp_slot_bytes(D));
    if (ga < 1) ga = 1;
    while (ga > 4 && (agents + ga - 1) / ga < (long long)FLP_WG_PER_CU * n_cu) ga >>= 1;
    return ga;
}

// elem_kind 0: float64, 1: int32.  FL_ERR_ARG (nothing launched) when the range has more workgroups than a grid holds
static inline int fl_launch_predict(const FlDev &d, const uint32_t *rcell, int b0, int nb, int D, int elem_kind, int n_cu, void *pred,
                                    int32_t *path, int32_t *path_len, hipStream_t s) {
    const long long agents = (long long)nb * d.A;
    const int ga = flp_shape(agents, D, n_cu);
    const long long wgs = (agents + ga - 1) / ga;
    if (wgs > 0x7FFFFFFFll) return FL_ERR_ARG;
    const size_t lds = flp_lds_bytes(ga, D);
    if (elem_kind == 0)
        hipLaunchKernelGGL(k_predict<double>, dim3((unsigned)wgs), dim3(FLP_THREADS), lds, s, d, rcell, b0, nb, D, ga, (double *)pred, path,
                           path_len);
    else
        hipLaunchKernelGGL(k_predict<int32_t>, dim3((unsigned)wgs), dim3(FLP_THREADS), lds, s, d, rcell, b0, nb, D, ga, (int32_t *)pred, path,
                           path_len);
    return FL_OK;
}
