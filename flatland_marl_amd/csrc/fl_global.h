// fl_global.h -- flatland.envs.observations.GlobalObsForRailEnv (observations.py:535-611) for a range of envs, one launch
// (gfx950).  Included by fl_host.hip, next to its entry point fl_obs_global.
//
// Per env b of the range, the reference returns for every handle
//   rail_obs     [H][W][16]  channel k = bit 15 - k of the cell's transitions (:560-566), one array for every handle
//   agents_state [H][W][5]   ch0 -1, the handle's direction at its virtual position (initial_position off the map, position on it,
//                            target when DONE); ch1 -1, the direction of every OTHER agent not DONE that has a position; ch2 / ch3 -1,
//                            malfunction_down_counter / speed of every agent not DONE that has a position; ch4 0, += 1 at the
//                            initial_position of every agent not DONE in an off-map state, the handle included (:568-611)
//   targets      [H][W][2]   ch0 1 at the handle's own target (also when DONE), ch1 1 at the target of every agent not DONE
// On-map positions are NOT unique: an agent whose malfunction ends off the map and that is told to stop is put on its
// initial_position without MotionCheck being asked (rail_env.py:599-601), onto whoever stands there.  The reference walks the agents in
// handle order and the last writer wins, so ch1..ch3 of a cell come from the HIGHEST handle on it, all three from that one agent.
// Every handle's two arrays are still ONE per-env slab -- ch0 all -1, ch1..ch4 and the targets' ch1 as above, targets' ch0 all 0 --
// with three single-cell patches: ch0 at the virtual position; ch1 of the handle's own cell when it is the highest handle there: -1,
// or the direction of the highest OTHER handle on that cell; the targets' ch0 at its own target.
//
// Kernel: one workgroup per (env, band of cells, group of agents).  A band is a run of consecutive cells (row-major, so every
// agent's band is one contiguous run of the output) sized to the LDS budget; the workgroup builds the band's slab in LDS (the highest
// handle of a cell with an LDS atomicMax, the ch4 counts with LDS float adds of 1, exact), then streams it once per agent of its group
// with the patches applied on the way -- 16-byte
// stores (plain: measured faster than non-temporal ones here, FLG_NT), scalar ones only where an agent's run starts or ends
// inside a 16-byte word.  The rail channels of a band are
// written by its group-0 workgroup.  Pure HBM write traffic: nothing is read back, the reads are the env's agents (A x 28 B) and
// the band's grid cells.
#pragma once
#include "fl_internal.h"

#ifndef FLG_THREADS
#define FLG_THREADS 256
#endif
#ifndef FLG_LDS_BUDGET
#define FLG_LDS_BUDGET (40 * 1024)   // bytes a workgroup: four workgroups (16 waves) a CU by LDS
#endif
#ifndef FLG_WG_PER_CU
#define FLG_WG_PER_CU 4              // agent groups are added until the grid has this many workgroups a CU
#endif
#ifndef FLG_NT
#define FLG_NT 0                     // 1: non-temporal output stores.  Same-box A/B (tools/global_obs_bench.py, two rounds): plain stores
#endif                               // cfg2 f32 36.5 -> 24.5 us, cfg3 f32 0.61 -> 0.52 ms; see profiles/global_obs_bench.json
template <typename V, typename P>
__device__ __forceinline__ void flg_store(V v, P *p) {
#if FLG_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

template <typename T> struct flg_vec;
template <> struct flg_vec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct flg_vec<double> { typedef double type __attribute__((ext_vector_type(2))); };

// Elements [seg0 + i * stride, + n) of out for the agents i = 0 .. na-1 of the group: slab[0 .. n) with slab[ka[i]] = va[i] and
// slab[kb[i]] = vb (ka / kb < 0: no patch; va == nullptr: the ka patch writes vb too).  KBV: kb[i] holds index * 8 + value + 1 with its
// own value -1 .. 3 instead of vb.  out is 16-byte aligned; one lane writes one aligned 16-byte word.
template <typename T, bool KBV>
__device__ __forceinline__ void flg_stream(T *__restrict__ out, size_t seg0, size_t stride, int na, int n, const T *slab,
                                           const int *ka, const T *va, const int *kb, T vb) {
    typedef typename flg_vec<T>::type VT;
    constexpr int V = 16 / sizeof(T);
    const int m = (n + V - 1) / V + 1;   // aligned words a run of n elements can touch
    for (int t = threadIdx.x; t < na * m; t += FLG_THREADS) {
        const int i = t / m, j = t - i * m;
        const size_t s = seg0 + (size_t)i * stride;
        const size_t gw = s / V + j;                       // aligned word of out
        const long long k0 = (long long)(gw * V) - (long long)s;   // local index of its first element (< 0 at a run's head)
        if (k0 >= n) continue;
        const int pa = ka[i], kbi = kb[i];
        const int pb = KBV ? kbi >> 3 : kbi;          // (-1 stays -1)
        const T xa = va != nullptr ? va[i] : vb;
        const T xb = KBV ? (T)((kbi & 7) - 1) : vb;
        if (k0 >= 0 && k0 + V <= n) {
            VT v;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const int k = (int)k0 + e;
                v[e] = k == pa ? xa : k == pb ? xb : slab[k];
            }
            flg_store(v, reinterpret_cast<VT *>(out + gw * V));
        } else {
#pragma unroll
            for (int e = 0; e < V; e++) {
                const long long k = k0 + e;
                if (k < 0 || k >= n) continue;
                const T x = k == pa ? xa : k == pb ? xb : slab[k];
                flg_store(x, out + gw * V + e);
            }
        }
    }
}

// grid (nb, bands, groups); dynamic LDS = flg_lds_bytes(cb, ga, sizeof(T))
template <typename T>
__global__ void __launch_bounds__(FLG_THREADS) k_obs_global(FlDev d, int b0, int cb, int ga, T *__restrict__ rail,
                                                            T *__restrict__ ast, T *__restrict__ tgt) {
    extern __shared__ __align__(16) unsigned char flg_lds[];
    const int A = d.A, HW = d.H * d.W;
    const int bl = blockIdx.x, b = b0 + bl;
    const int c0 = blockIdx.y * cb, nc = min(cb, HW - c0);
    const int a0 = blockIdx.z * ga, na = min(ga, A - a0);
    if (nc <= 0 || na <= 0) return;
    T *s_as = reinterpret_cast<T *>(flg_lds);     // [cb][5]
    T *s_tg = s_as + (size_t)cb * 5;               // [cb][2]
    T *s_dir = s_tg + (size_t)cb * 2;              // [ga] the agents' directions (ch0 patch value)
    int *s_top = reinterpret_cast<int *>(s_dir + ga);             // [cb] 1 + the highest handle that stands on the cell (0: none)
    int *s_k0 = s_top + cb;                                        // [ga] ch0 patch (local element index, -1 = none)
    int *s_k1 = s_k0 + ga;                                         // [ga] ch1 patch: index * 8 + value + 1 (flg_stream KBV), -1 = none
    int *s_kt = s_k1 + ga;                                         // [ga] targets' ch0
    __shared__ int s_stacked;                                      // some cell of the band holds more than one train
    const int tid = threadIdx.x;

    // rail channels of the band (observations.py:560-566): group 0 only; 16 elements a cell -> whole aligned words
    if (rail != nullptr && blockIdx.z == 0) {
        typedef typename flg_vec<T>::type VT;
        constexpr int V = 16 / sizeof(T);
        const uint32_t *grid = d.grid + (size_t)d.tab[b] * HW;     // (envs with one map share one set of slabs, FlDev::tab)
        T *out = rail + ((size_t)bl * HW + c0) * 16;
        for (int w = tid; w < nc * (16 / V); w += FLG_THREADS) {
            const int cell = w / (16 / V), k = (w % (16 / V)) * V;
            const uint32_t bits = grid[c0 + cell];
            VT v;
#pragma unroll
            for (int e = 0; e < V; e++) v[e] = (T)((bits >> (15 - k - e)) & 1u);
            flg_store(v, reinterpret_cast<VT *>(out) + w);
        }
    }
    if (ast == nullptr && tgt == nullptr) return;

    for (int i = tid; i < nc * 5; i += FLG_THREADS) s_as[i] = (i % 5) == 4 ? (T)0 : (T)-1;
    for (int i = tid; i < nc * 2; i += FLG_THREADS) s_tg[i] = (T)0;
    for (int i = tid; i < nc; i += FLG_THREADS) s_top[i] = 0;
    if (tid == 0) s_stacked = 0;
    __syncthreads();

    // the env-wide part (:592-610), first half: the targets, the ch4 counts, every cell's highest handle; the group's ch0 / target patches
    const size_t g0 = (size_t)b * A;
    uint32_t pk_r = 0;                  // the lane's first agent (a = tid: every agent when A <= 256) stays in registers for the second half
    int pos_r = -1;
    T malf_r = (T)0, speed_r = (T)0;
    for (int a = tid; a < A; a += FLG_THREADS) {
        const uint32_t pk = d.pk[g0 + a], st = PK_STATE(pk);
        const int pos = d.pos[g0 + a], ip = d.init_pos[g0 + a], tg = d.target[g0 + a];
        const int lp = pos - c0, li = ip - c0, lt = tg - c0;
        if (a == tid) { pk_r = pk; pos_r = pos; }
        if (st != ST_DONE) {
            if (lt >= 0 && lt < nc) s_tg[lt * 2 + 1] = (T)1;
            if (pos >= 0 && lp >= 0 && lp < nc) {
                if (atomicMax(&s_top[lp], a + 1) != 0) s_stacked = 1;
                if (a == tid) { malf_r = (T)(d.malf[g0 + a] & 0xFFFFu); speed_r = (T)d.speed[g0 + a]; }
            }
            if (is_off_map(st) && li >= 0 && li < nc) atomicAdd(&s_as[li * 5 + 4], (T)1);
        }
        const int i = a - a0;
        if (i >= 0 && i < na) {
            const int lv = (is_off_map(st) ? ip : st == ST_DONE ? tg : pos) - c0;     // the virtual position (:572-579)
            s_k0[i] = lv >= 0 && lv < nc ? lv * 5 : -1;
            s_kt[i] = lt >= 0 && lt < nc ? lt * 2 : -1;
            s_dir[i] = (T)PK_DIR(pk);
        }
    }
    __syncthreads();
    // second half: a cell's ch1..ch3 from its highest handle (the reference's last writer); the ch1 patch of a group agent that IS the
    // highest handle of its cell -- what the handles below it left there: nothing, unless the band holds a stack
    const bool stacked = s_stacked != 0;
    for (int a = tid; a < A; a += FLG_THREADS) {
        const bool kept = a == tid;
        const uint32_t pk = kept ? pk_r : d.pk[g0 + a];
        const int pos = kept ? pos_r : d.pos[g0 + a], lp = pos - c0;
        const bool here = PK_STATE(pk) != ST_DONE && pos >= 0 && lp >= 0 && lp < nc;
        const bool top = here && s_top[lp] == a + 1;
        if (top) {
            s_as[lp * 5 + 1] = (T)PK_DIR(pk);
            s_as[lp * 5 + 2] = kept ? malf_r : (T)(d.malf[g0 + a] & 0xFFFFu);
            s_as[lp * 5 + 3] = kept ? speed_r : (T)d.speed[g0 + a];
        }
        const int i = a - a0;
        if (i >= 0 && i < na) {
            int v = -1;
            if (top && stacked)
                for (int j = a - 1; j >= 0; j--) {     // the highest OTHER handle on the cell
                    const uint32_t pj = d.pk[g0 + j];
                    if (d.pos[g0 + j] == pos && PK_STATE(pj) != ST_DONE) { v = (int)PK_DIR(pj); break; }
                }
            s_k1[i] = top ? (lp * 5 + 1) * 8 + v + 1 : -1;
        }
    }
    __syncthreads();

    const size_t first = (size_t)bl * A + a0;     // the group's first agent in the range's [nb][A] order
    if (ast != nullptr)
        flg_stream<T, true>(ast, first * HW * 5 + (size_t)c0 * 5, (size_t)HW * 5, na, nc * 5, s_as, s_k0, s_dir, s_k1, (T)-1);
    if (tgt != nullptr)
        flg_stream<T, false>(tgt, first * HW * 2 + (size_t)c0 * 2, (size_t)HW * 2, na, nc * 2, s_tg, s_kt, nullptr, s_kt, (T)1);
}

static inline size_t flg_lds_bytes(int cb, int ga, int eb) { return (size_t)cb * (7 * eb + 4) + (size_t)ga * (eb + 12); }

// Launch shape for nb envs of A agents on HW cells: bands of at most the LDS budget, then agent groups until the grid has about
// four workgroups a CU.
static inline void flg_shape(int nb, int A, int HW, int eb, int n_cu, int *cb, int *bands, int *ga, int *groups) {
    const long long per_cell = 7 * eb + 4, per_agent = eb + 12;
    long long cmax = ((long long)FLG_LDS_BUDGET - per_agent * A) / per_cell;
    if (cmax < 64) cmax = 64;
    int nbd = (int)((HW + cmax - 1) / cmax);
    long long wg = (long long)nb * nbd;
    int ng = 1;
    if (wg < (long long)FLG_WG_PER_CU * n_cu) ng = (int)std::min<long long>(((long long)FLG_WG_PER_CU * n_cu + wg - 1) / wg, (A + 3) / 4);
    if (ng < 1) ng = 1;
    *ga = (A + ng - 1) / ng;
    *groups = (A + *ga - 1) / *ga;
    *cb = (HW + nbd - 1) / nbd;
    *bands = (HW + *cb - 1) / *cb;
}

// FL_ERR_ARG (nothing launched) when the map has more bands than a grid dimension holds
static inline int fl_launch_obs_global(const FlDev &d, int b0, int nb, int eb, int n_cu, void *rail, void *ast, void *tgt,
                                       hipStream_t s) {
    int cb, bands, ga, groups;
    flg_shape(nb, d.A, d.H * d.W, eb, n_cu, &cb, &bands, &ga, &groups);
    if (bands > 65535) return FL_ERR_ARG;
    const bool per_agent = ast != nullptr || tgt != nullptr;
    const dim3 grid(nb, bands, per_agent ? groups : 1);      // (the rail alone: no slab, nothing per agent)
    const size_t lds = per_agent ? flg_lds_bytes(cb, ga, eb) : 0;
    if (eb == 8)
        hipLaunchKernelGGL(k_obs_global<double>, grid, dim3(FLG_THREADS), lds, s, d, b0, cb, ga, (double *)rail, (double *)ast,
                           (double *)tgt);
    else
        hipLaunchKernelGGL(k_obs_global<float>, grid, dim3(FLG_THREADS), lds, s, d, b0, cb, ga, (float *)rail, (float *)ast,
                           (float *)tgt);
    return FL_OK;
}
