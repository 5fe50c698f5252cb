// fl_wrappers.h -- the reduced action space of flatland/contrib/wrappers/flatland_wrappers.py for a range of envs (gfx950):
//   possible_actions_sorted_by_distance(env, handle)  (:14-56)     the candidate list of every agent
//   ShortestPathActionWrapper.step                     (:122-141)   reduced action {0, 1, 2} -> RailEnvActions
//   find_all_cells_where_agent_can_choose(env)         (:145-176)   switches and their neighbours, one byte a cell
//   SkipNoChoiceCellsWrapper.on_decision_cell          (:197-198)   the flag that hands an agent back to the policy
// Included by fl_host.hip, next to its entry points fl_action_space and fl_decision_cells (include/flatland_wrappers.h).
//
// k_decision_cells is static per map: cellkind u8 [B][H*W], bit 0 = switch (some orientation of the cell has more than one
// transition), bit 1 = switch neighbour (the cell is get_new_position(s, m) of a switch s and a transition m that s has in any of
// its orientations).  Bit 1 is a GATHER: cell c looks at its four neighbours c + step(k) and asks whether that cell is a switch
// with a transition of movement (k + 2) % 4 -- no atomics, no scatter.  Cells without rail get 0 (the reference's sets also hold
// the empty or off-map cells a malformed switch points at; no agent can stand there).  Only the slabs of the table owners
// (FlDev::tab) are built: env b reads slab tab[b].  It depends on the rail grid alone, so it is launched where the grid's tables
// are (re)built -- the commit and the full rebuild -- and not by a masked distance-map rebuild, which leaves the grid as it is.
//
// k_action_space runs per step, one lane per agent of the envs [b0, b0 + nb): about a dozen table reads (pk, pos, init_pos,
// tslot, tab, grid, up to three of ridx and dm, cellkind, reduced) and under 40 bytes written.  Nothing to tile: the launch is
// latency-bound.  Every loop is bounded by 4, every table index comes from a table or is checked against HW / Rcap / Ucap,
// nothing is written outside the given outputs.
//
// Where the reference leaves the path the kernel is defined as follows:
//   - a reduced action a >= 1 with a - 1 >= count: the reference raises IndexError, the kernel writes DO_NOTHING (0)
//   - a neighbour off the grid or without rail: distance infinity (the reference's value off the grid is an accident of numpy's
//     negative indexing; valid maps have no such neighbour)
//   - an on-map agent on a cell without any transition for its direction (no valid map): the reference returns [], the kernel
//     count 0; four transitions for one direction (no Flatland cell type): the kernel keeps the three nearest, count 3
#pragma once
#include "fl_internal.h"

#ifndef FLW_THREADS
#define FLW_THREADS 256
#endif
#define FLW_SLOTS 3   // entries a candidate list holds

// is the 16-bit cell a switch / has it a transition of movement m in any orientation
__device__ __forceinline__ bool flw_is_switch(uint32_t cell) {
    bool sw = false;
#pragma unroll
    for (uint32_t o = 0; o < 4; o++) sw |= __popc(nibble(cell, o)) > 1;
    return sw;
}
__device__ __forceinline__ bool flw_moves(uint32_t cell, uint32_t m) { return ((cell | (cell >> 4) | (cell >> 8) | (cell >> 12)) >> (3u - m)) & 1u; }

// grid (B * nblk), nblk = ceil(H * W / FLW_THREADS): one lane a cell; mask: u8 [B] or nullptr (= every env)
__global__ void __launch_bounds__(FLW_THREADS) k_decision_cells(FlDev d, const uint8_t *__restrict__ mask, int nblk, uint8_t *__restrict__ cellkind) {
    const int b = blockIdx.x / nblk, H = d.H, W = d.W, HW = H * W;
    if (b >= d.B || (mask != nullptr && mask[b] == 0)) return;
    const int c = (blockIdx.x - b * nblk) * FLW_THREADS + threadIdx.x;
    if (c >= HW) return;
    const uint32_t *grid = d.grid + (size_t)b * HW;
    const uint32_t cell = grid[c] & 0xFFFFu;
    uint32_t kind = 0;
    if (cell != 0) {
        kind = flw_is_switch(cell) ? 1u : 0u;
        const int row = c / W, col = c - row * W;
        bool nb = false;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const int nr = row + (k == 0 ? -1 : k == 2 ? 1 : 0), nc = col + (k == 1 ? 1 : k == 3 ? -1 : 0);
            if (nr < 0 || nr >= H || nc < 0 || nc >= W) continue;
            const uint32_t n = grid[nr * W + nc] & 0xFFFFu;
            nb |= flw_is_switch(n) && flw_moves(n, (k + 2u) & 3u);
        }
        kind |= nb ? 2u : 0u;
    }
    cellkind[(size_t)b * HW + c] = (uint8_t)kind;
}

static inline void fl_launch_decision_cells(const FlDev &d, const uint8_t *mask_dev, uint8_t *cellkind, hipStream_t s) {
    const int nblk = (d.H * d.W + FLW_THREADS - 1) / FLW_THREADS;
    hipLaunchKernelGGL(k_decision_cells, dim3((unsigned)((long long)d.B * nblk)), dim3(FLW_THREADS), 0, s, d, mask_dev, nblk, cellkind);
}

// grid (nb * nblk): cells u8 [nb][H*W] = the slab of each env's table owner
__global__ void __launch_bounds__(FLW_THREADS) k_decision_cells_out(FlDev d, const uint8_t *__restrict__ cellkind, int b0, int nb, int nblk,
                                                                    uint8_t *__restrict__ cells) {
    const int HW = d.H * d.W;
    const int e = blockIdx.x / nblk;
    const int c = (blockIdx.x - e * nblk) * FLW_THREADS + threadIdx.x;
    if (e >= nb || c >= HW) return;
    const int tb = d.tab[b0 + e];
    cells[(size_t)e * HW + c] = cellkind[(size_t)tb * HW + c];
}

static inline void fl_launch_decision_cells_out(const FlDev &d, const uint8_t *cellkind, int b0, int nb, uint8_t *cells, hipStream_t s) {
    const int nblk = (d.H * d.W + FLW_THREADS - 1) / FLW_THREADS;
    hipLaunchKernelGGL(k_decision_cells_out, dim3((unsigned)((long long)nb * nblk)), dim3(FLW_THREADS), 0, s, d, cellkind, b0, nb, nblk, cells);
}

template <typename T> struct flw_inf;
template <> struct flw_inf<double> { __device__ static double value() { return __builtin_huge_val(); } };
template <> struct flw_inf<int32_t> { __device__ static int32_t value() { return 0x7FFFFFFF; } };

// grid (ceil(nb * A / wg)), wg lanes a workgroup.  sp_action u8 [nb][A][3], sp_dist T [nb][A][3], sp_count u8 [nb][A]: all three or
// none; on_decision u8 [nb][A] or nullptr; reduced / actions u8 [nb][A]: both or neither.
template <typename T>
__global__ void __launch_bounds__(FLW_THREADS) k_action_space(FlDev d, const uint8_t *__restrict__ cellkind, int b0, int nb,
                                                              uint8_t *__restrict__ sp_action, T *__restrict__ sp_dist,
                                                              uint8_t *__restrict__ sp_count, uint8_t *__restrict__ on_decision,
                                                              const uint8_t *__restrict__ reduced, uint8_t *__restrict__ actions) {
    const int A = d.A, H = d.H, W = d.W, HW = H * W, Rcap = d.Rcap;
    const long long total = (long long)nb * A;
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // the agent in the range's [nb][A] order
    if (q >= total) return;
    const size_t g = (size_t)b0 * A + (size_t)q;
    const int b = (int)(g / A), tb = d.tab[b];
    const uint32_t pk = d.pk[g], state = PK_STATE(pk), dir = PK_DIR(pk);
    const int pos = d.pos[g], ipos = d.init_pos[g];
    const bool on_map = is_on_map(state);

    if (on_decision != nullptr) {
        // position is None off the map and when DONE (flatland_wrappers.py:197-198)
        bool dec = !on_map || pos == ipos;
        if (!dec && pos >= 0 && pos < HW) dec = cellkind[(size_t)tb * HW + pos] != 0;
        on_decision[q] = dec ? 1 : 0;
    }
    if (sp_action == nullptr && actions == nullptr) return;

    // ---- the candidates in N, E, S, W order (flatland_wrappers.py:28-48), then the stable sort by distance (:49)
    // (fully unrolled on purpose: every array index is a constant, so the four candidates stay in registers)
    uint32_t act[FLW_SLOTS] = {0, 0, 0}, dist[FLW_SLOTS] = {FL_INF16, FL_INF16, FL_INF16};
    int count = 2;
    const int vpos = state == ST_READY ? ipos : on_map ? pos : -1;
    if (vpos >= 0 && vpos < HW) {
        const uint32_t bits = nibble(d.grid[(size_t)tb * HW + vpos] & 0xFFFFu, dir);
        const int u = d.tslot[g];
        const bool have_dm = u >= 0 && u < d.Ucap;
        const uint16_t *dm = d.dm + ((size_t)tb * d.Ucap + (have_dm ? u : 0)) * ((size_t)Rcap * 4);
        const uint16_t *ridx = d.ridx + (size_t)tb * HW;
        const int row = vpos / W, col = vpos - row * W;
        bool cv[4];
        uint32_t ca[4], cd[4];
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) {
            cv[m] = (bits >> (3u - m)) & 1u;
            ca[m] = m == dir ? ACT_FORWARD : m == ((dir + 1u) & 3u) ? ACT_RIGHT : m == ((dir + 3u) & 3u) ? ACT_LEFT : ACT_FORWARD;
            const int nr = row + (m == 0 ? -1 : m == 2 ? 1 : 0), nc = col + (m == 1 ? 1 : m == 3 ? -1 : 0);
            cd[m] = FL_INF16;
            if (cv[m] && have_dm && nr >= 0 && nr < H && nc >= 0 && nc < W) {
                const uint32_t r = ridx[nr * W + nc];
                if (r < (uint32_t)Rcap) cd[m] = dm[(size_t)r * 4 + m];
            }
        }
        // the stable sort as ranks: candidate m goes behind every candidate that is nearer, or as near and earlier in N, E, S, W
        int n = 0;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) rank += cv[j] && (cd[j] < cd[m] || (cd[j] == cd[m] && j < m));
            n += cv[m];
#pragma unroll
            for (int k = 0; k < FLW_SLOTS; k++)
                if (cv[m] && rank == k) { act[k] = ca[m]; dist[k] = cd[m]; }
        }
        if (n == 1) { act[1] = act[0]; dist[1] = dist[0]; }
        count = n == 1 ? 2 : n > FLW_SLOTS ? FLW_SLOTS : n;
    } else if (!on_map && state != ST_READY) {
        dist[0] = dist[1] = 0;      // [(DO_NOTHING, 0)] * 2 (flatland_wrappers.py:26)
    } else {
        count = 0;                  // (a position outside the grid: no valid state)
    }

    if (sp_action != nullptr) {
#pragma unroll
        for (int k = 0; k < FLW_SLOTS; k++) {
            const bool in = k < count;
            sp_action[(size_t)q * FLW_SLOTS + k] = (uint8_t)(in ? act[k] : 0u);
            sp_dist[(size_t)q * FLW_SLOTS + k] = in && dist[k] != FL_INF16 ? (T)dist[k] : flw_inf<T>::value();
        }
        sp_count[q] = (uint8_t)count;
    }
    if (actions != nullptr) {
        // ShortestPathActionWrapper.step (flatland_wrappers.py:131-138); an agent absent from the dict stays absent
        const uint32_t a = reduced[q];
        uint32_t out = a;
        if (a != 255u && a != 0u) {
            const uint32_t k = a - 1u;
            out = k < (uint32_t)count ? (k == 0 ? act[0] : k == 1 ? act[1] : act[2]) : (uint32_t)ACT_NOTHING;
        }
        actions[q] = (uint8_t)out;
    }
}

// lanes a workgroup: halved from FLW_THREADS down to one wavefront while the grid has fewer workgroups than the device has CUs
static inline int flw_shape(long long agents, int n_cu) {
    int wg = FLW_THREADS;
    while (wg > 64 && (agents + wg - 1) / wg < (long long)n_cu) wg >>= 1;
    return wg;
}

// elem_kind 0: float64, 1: int32.  FL_ERR_ARG (nothing launched) when the range has more workgroups than a grid holds
static inline int fl_launch_action_space(const FlDev &d, const uint8_t *cellkind, int b0, int nb, int elem_kind, int n_cu, uint8_t *sp_action,
                                         void *sp_dist, uint8_t *sp_count, uint8_t *on_decision, const uint8_t *reduced, uint8_t *actions,
                                         hipStream_t s) {
    const long long agents = (long long)nb * d.A;
    const int wg = flw_shape(agents, n_cu);
    const long long wgs = (agents + wg - 1) / wg;
    if (wgs > 0x7FFFFFFFll) return FL_ERR_ARG;
    if (elem_kind == 0)
        hipLaunchKernelGGL(k_action_space<double>, dim3((unsigned)wgs), dim3(wg), 0, s, d, cellkind, b0, nb, sp_action, (double *)sp_dist, sp_count,
                           on_decision, reduced, actions);
    else
        hipLaunchKernelGGL(k_action_space<int32_t>, dim3((unsigned)wgs), dim3(wg), 0, s, d, cellkind, b0, nb, sp_action, (int32_t *)sp_dist, sp_count,
                           on_decision, reduced, actions);
    return FL_OK;
}
