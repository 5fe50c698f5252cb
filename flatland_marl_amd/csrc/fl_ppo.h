// fl_ppo.h -- the kernels of include/flatland_ppo.h: the per-row draw with its log-probability and entropy (k_policy_sample), the
// PPO loss with its gradients (k_ppo_count, k_ppo_rows, k_ppo_final) and generalised advantage estimation (k_gae), gfx950.
// Included by fl_policy_head.hip behind fl_policy_head.h, whose fph_choose is the draw.
//
// Rows = the (env, agent) pairs, one lane a row, 256 rows a workgroup.  A row is 20 bytes of logits and 5 of mask, so a workgroup's
// rows are one span of 5 KB + 1.25 KB: it is read as whole dwords / bytes by consecutive lanes into LDS (fpp_stage) and a lane
// takes its row from there (row stride 5 dwords: odd, conflict-free); the gradient rows leave the same way.  Everything a row
// computes is float64 (5 exp and a log for the log-softmax, one more exp for rho) from its float32 inputs.
//
// The loss is three launches on one stream, no float atomic, no integer atomic either:
//   k_ppo_count   at most FPP_COUNT_GROUPS workgroups stride over the rows and leave (counted rows, rows whose action is not valid)
//                 per workgroup: n is needed before a gradient can be scaled by 1 / n
//   k_ppo_rows    a workgroup adds those counts (integers: any order gives n), then writes its 256 gradient rows and 256 value
//                 gradients and leaves its five float64 sums in ITS slot of the workspace (fpp_block_sum: a fixed tree)
//   k_ppo_final   one workgroup: lane t adds the slots t, t + 256, ... in index order, the same tree, the eight statistics
// so every address has one writer and the bits do not depend on the order the workgroups ran in.
#pragma once
#include "fl_policy_head.h"

#define FPP_THREADS 256
#define FPP_COUNT_GROUPS 1024       // the most workgroups of k_ppo_count = the most count slots a workgroup of k_ppo_rows adds
#define FPP_SUMS 5                  // sum w s, sum w H, sum w (old_logp - logp_a), sum w [|rho - 1| > eps], sum (v - R)^2

struct FppLossArgs {
    int R, B;                       // rows, values (0: no critic terms)
    int groups, count_groups;       // workgroups of k_ppo_rows / of k_ppo_count
    const float *logits;
    const unsigned char *valid, *actions, *mask;
    const float *old_logp, *adv, *value, *returns;
    double clip_eps, vf_coef, ent_coef;
    float *grad_logits, *grad_value;
    double *stats;
    double *sums;                   // workspace: [groups][FPP_SUMS]
    int *counts;                    // workspace: [count_groups][2]
};

// the sum of v over the workgroup's 256 threads in a fixed tree: a wavefront's 64 lanes by halving, the four wavefronts in order.
// Every thread gets the sum; `lds` holds 4 values and is free again on return
template <class T>
__device__ __forceinline__ T fpp_block_sum(T v, T *lds) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// the workgroup's rows [row0, row0 + 256) of logits and mask into LDS, consecutive lanes reading consecutive dwords / bytes
__device__ __forceinline__ void fpp_stage(float *s_lg, unsigned char *s_va, const float *logits, const unsigned char *valid, int row0, int R) {
    const size_t base = (size_t)row0 * FPH_ACT, end = (size_t)R * FPH_ACT;
    for (int k = 0; k < FPH_ACT; k++) {
        const int i = threadIdx.x + FPP_THREADS * k;
        if (base + i < end) { s_lg[i] = logits[base + i]; s_va[i] = valid[base + i]; }
    }
    __syncthreads();
}

// the float64 log-softmax of one row over its valid actions, the sums in ascending j: logp_j, p_j (0 where j is not valid), the
// entropy H = - sum p_j logp_j; returns the number of valid actions (0: everything 0)
__device__ __forceinline__ int fpp_log_softmax(const float *x, const unsigned char *valid, double (&logp)[FPH_ACT], double (&p)[FPH_ACT],
                                               double &H) {
    int nv = 0;
    double m = 0.0;
    for (int j = 0; j < FPH_ACT; j++)
        if (valid[j]) { m = nv ? fmax(m, (double)x[j]) : (double)x[j]; nv++; }
    double e[FPH_ACT], S = 0.0;
    for (int j = 0; j < FPH_ACT; j++) {
        e[j] = valid[j] ? exp((double)x[j] - m) : 0.0;
        if (valid[j]) S += e[j];
    }
    const double logS = nv ? log(S) : 0.0;
    double acc = 0.0;
    for (int j = 0; j < FPH_ACT; j++) {
        logp[j] = valid[j] ? ((double)x[j] - m) - logS : 0.0;
        p[j] = valid[j] ? e[j] / S : 0.0;
        if (valid[j]) acc += p[j] * logp[j];
    }
    H = 0.0 - acc;
    return nv;
}

// ---- fl_policy_sample
__global__ void __launch_bounds__(FPP_THREADS) k_policy_sample(int R, const float *logits, const unsigned char *valid, const double *u,
                                                               unsigned char *actions, float *logp_out, float *entropy_out) {
    __shared__ float s_lg[FPP_THREADS * FPH_ACT];
    __shared__ unsigned char s_va[FPP_THREADS * FPH_ACT];
    const int row0 = blockIdx.x * FPP_THREADS, r = row0 + threadIdx.x;
    fpp_stage(s_lg, s_va, logits, valid, row0, R);
    if (r >= R) return;
    const float *x = s_lg + threadIdx.x * FPH_ACT;
    const unsigned char *va = s_va + threadIdx.x * FPH_ACT;
    const int a = fph_choose(x, va, 1, u[r]);
    actions[r] = (unsigned char)a;
    if (!logp_out && !entropy_out) return;
    double logp[FPH_ACT], p[FPH_ACT], H;
    const int nv = fpp_log_softmax(x, va, logp, p, H);
    double la = 0.0;
    for (int j = 0; j < FPH_ACT; j++)
        if (j == a) la = logp[j];
    if (logp_out) logp_out[r] = nv ? (float)la : 0.f;
    if (entropy_out) entropy_out[r] = (float)H;
}

// ---- fl_ppo_loss
// 1 = the row is counted, 2 = it is left out for its action alone (not masked, a valid action exists, the action is not one)
__device__ __forceinline__ int fpp_row_class(const unsigned char *valid, unsigned a, bool masked_out) {
    bool any = false, ok = false;
    for (int j = 0; j < FPH_ACT; j++) {
        any |= valid[j] != 0;
        ok |= valid[j] != 0 && (unsigned)j == a;
    }
    if (masked_out || !any) return 0;
    return ok ? 1 : 2;
}

__global__ void __launch_bounds__(FPP_THREADS) k_ppo_count(FppLossArgs p) {
    __shared__ int s_red[4];
    int n = 0, bad = 0;
    for (int r = blockIdx.x * FPP_THREADS + threadIdx.x; r < p.R; r += p.count_groups * FPP_THREADS) {
        const int c = fpp_row_class(p.valid + (size_t)r * FPH_ACT, p.actions[r], p.mask && p.mask[r] == 0);
        n += c == 1;
        bad += c == 2;
    }
    n = fpp_block_sum(n, s_red);
    bad = fpp_block_sum(bad, s_red);
    if (threadIdx.x == 0) { p.counts[2 * blockIdx.x] = n; p.counts[2 * blockIdx.x + 1] = bad; }
}

// the counts of k_ppo_count added up: every thread gets (n, rows whose action is not valid)
__device__ __forceinline__ void fpp_counts(const FppLossArgs &p, int *s_red, int &n, int &bad) {
    n = 0; bad = 0;
    for (int i = threadIdx.x; i < p.count_groups; i += FPP_THREADS) { n += p.counts[2 * i]; bad += p.counts[2 * i + 1]; }
    n = fpp_block_sum(n, s_red);
    bad = fpp_block_sum(bad, s_red);
}

__global__ void __launch_bounds__(FPP_THREADS) k_ppo_rows(FppLossArgs p) {
    __shared__ float s_lg[FPP_THREADS * FPH_ACT];
    __shared__ unsigned char s_va[FPP_THREADS * FPH_ACT];
    __shared__ double s_red[4];
    int n, bad;
    fpp_counts(p, (int *)s_red, n, bad);
    const int row0 = blockIdx.x * FPP_THREADS, r = row0 + threadIdx.x;
    double sum[FPP_SUMS] = {};
    float g[FPH_ACT] = {};
    if (row0 < p.R) fpp_stage(s_lg, s_va, p.logits, p.valid, row0, p.R);
    if (r < p.R) {
        const float *x = s_lg + threadIdx.x * FPH_ACT;
        const unsigned char *va = s_va + threadIdx.x * FPH_ACT;
        const unsigned a = p.actions[r];
        if (fpp_row_class(va, a, p.mask && p.mask[r] == 0) == 1) {
            double logp[FPH_ACT], pr[FPH_ACT], H;
            fpp_log_softmax(x, va, logp, pr, H);
            double la = 0.0;
            for (int j = 0; j < FPH_ACT; j++)
                if ((unsigned)j == a) la = logp[j];
            const double old = (double)p.old_logp[r], A = (double)p.adv[r];
            const double lo = 1.0 - p.clip_eps, hi = 1.0 + p.clip_eps;
            const double rho = exp(la - old);
            const double s = fmin(rho * A, fmin(fmax(rho, lo), hi) * A);
            const double gs = ((A >= 0.0 && rho <= hi) || (A < 0.0 && rho >= lo)) ? rho * A : 0.0;
            sum[0] = s; sum[1] = H; sum[2] = old - la; sum[3] = fabs(rho - 1.0) > p.clip_eps ? 1.0 : 0.0;
            for (int j = 0; j < FPH_ACT; j++)
                if (va[j]) {
                    const double d = (unsigned)j == a ? 1.0 : 0.0;
                    g[j] = (float)((-gs * (d - pr[j]) + p.ent_coef * (pr[j] * (logp[j] + H))) / (double)n);
                }
        }
    }
    if (row0 < p.R) {                                  // the gradient rows leave as they came: through LDS, whole dwords in lane order
        __syncthreads();
        for (int j = 0; j < FPH_ACT; j++) s_lg[threadIdx.x * FPH_ACT + j] = g[j];
        __syncthreads();
        const size_t base = (size_t)row0 * FPH_ACT, end = (size_t)p.R * FPH_ACT;
        for (int k = 0; k < FPH_ACT; k++) {
            const int i = threadIdx.x + FPP_THREADS * k;
            if (base + i < end) p.grad_logits[base + i] = s_lg[i];
        }
    }
    if (r < p.B) {                                     // this workgroup's 256 values
        const double d = (double)p.value[r] - (double)p.returns[r];
        p.grad_value[r] = (float)(p.vf_coef * d / (double)p.B);
        sum[4] = d * d;
    }
    for (int q = 0; q < FPP_SUMS; q++) {
        const double t = fpp_block_sum(sum[q], s_red);
        if (threadIdx.x == 0) p.sums[(size_t)blockIdx.x * FPP_SUMS + q] = t;
    }
}

__global__ void __launch_bounds__(FPP_THREADS) k_ppo_final(FppLossArgs p) {
    __shared__ double s_red[4];
    int n, bad;
    fpp_counts(p, (int *)s_red, n, bad);
    double tot[FPP_SUMS];
    for (int q = 0; q < FPP_SUMS; q++) {
        double t = 0.0;
        for (int i = threadIdx.x; i < p.groups; i += FPP_THREADS) t += p.sums[(size_t)i * FPP_SUMS + q];
        tot[q] = fpp_block_sum(t, s_red);
    }
    if (threadIdx.x != 0) return;
    const double dn = (double)n;
    const double l_pi = n ? -tot[0] / dn : 0.0, h = n ? tot[1] / dn : 0.0;
    const double l_v = p.B ? 0.5 * (tot[4] / (double)p.B) : 0.0;
    p.stats[0] = l_pi;
    p.stats[1] = l_v;
    p.stats[2] = h;
    p.stats[3] = (l_pi + p.vf_coef * l_v) - p.ent_coef * h;
    p.stats[4] = n ? tot[2] / dn : 0.0;
    p.stats[5] = n ? tot[3] / dn : 0.0;
    p.stats[6] = dn;
    p.stats[7] = (double)bad;
}

// ---- fl_gae: a lane a column, the T steps from the last to the first.  The step's loads are coalesced across the lanes and do not
// depend on the carried A, so those of step t - 1 are issued before step t's arithmetic; the chain of T dependent float64
// operations is what the kernel takes: latency-bound over T by construction
__global__ void __launch_bounds__(FPP_THREADS) k_gae(int T, int N, const float *rew, const float *val, const unsigned char *dones, double gamma,
                                                     double lam, float *adv, float *ret) {
    const int c = blockIdx.x * FPP_THREADS + threadIdx.x;
    if (c >= N) return;
    size_t at = (size_t)(T - 1) * N + c;
    float r = rew[at], v0 = val[at], v1 = val[at + N];
    unsigned char d = dones[at];
    double A = 0.0;
    const double gl = gamma * lam;
    for (int t = T - 1; t >= 0; t--, at -= N) {
        float rn = 0.f, vn = 0.f;
        unsigned char dn = 0;
        if (t > 0) { rn = rew[at - N]; vn = val[at - N]; dn = dones[at - N]; }
        const double nd = d ? 0.0 : 1.0;
        const double delta = ((double)r + (gamma * (double)v1) * nd) - (double)v0;
        A = delta + (gl * nd) * A;
        adv[at] = (float)A;
        ret[at] = (float)(A + (double)v0);
        v1 = v0; r = rn; v0 = vn; d = dn;
    }
}
