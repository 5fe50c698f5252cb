// fl_obs_index.h -- the small device helpers of the per-key prediction index (phase 2 of obs_body, fl_obs_body.h; pass B's own-path
// filter, fl_obs_passb.h): the predictors' timing, the bucket-range mask, the packed bucket counters, the fetch of a waypoint's path words.
#pragma once
#include "fl_obs_ctx.h"

// Closed time interval [tlo, thi()] (span times) during which an agent is predicted on waypoint k: lp its last indexed waypoint, tpc its
// times per cell, tlast the last predicted time.  flatland_cutils (predictions.cpp:78-235): w(t) = 0 for t = 0, min((t - 1) / tpc + 1, lp)
// afterwards; upstream (predictions.py:97-180): w(t) = min(t / tpc, lp).  to_end: the agent stays until the end of the horizon.
// (thi() is formed where it is used: the kernels sit at their register ceiling, and a value kept from here to there costs spills.)
struct WpInterval {
    int tlo, span, tlast;
    bool to_end;
    __device__ __forceinline__ int thi() const { return to_end ? tlast : tlo + span - 1; }
};
template <bool CUTILS>
__device__ __forceinline__ WpInterval wp_interval(int k, int lp, int tpc, int tlast) {
    WpInterval v;
    v.tlast = tlast;
    v.tlo = CUTILS ? (k == 0 ? 0 : (k - 1) * tpc + 1) : k * tpc;
    v.span = (CUTILS && k == 0) ? 1 : tpc;
    v.to_end = k == lp || v.tlo + v.span - 1 >= tlast;
    return v;
}
// bits b1 .. b2 (b1 <= b2 <= 63) of a per-key time mask: the buckets tb_of(tlo) .. tb_of(thi) of an item
__device__ __forceinline__ unsigned long long bucket_range_mask(int b1, int b2) { return ((2ull << b2) - 1ull) & ~((1ull << b1) - 1ull); }
// Per-(key, bucket) counters of the bucketed lists, 16 bits each: counter kb is half kb & 1 of word kb >> 1.  half_count_bump returns the
// count before it (the item's slot in the bucket) = half_count_of(half_count_add()), for a site with work between the two; _drop takes one back.
__device__ __forceinline__ uint32_t half_count_add(uint32_t *c, int kb) { return atomicAdd(&c[kb >> 1], (kb & 1) ? 0x10000u : 1u); }
__device__ __forceinline__ uint32_t half_count_of(uint32_t word, int kb) { return (kb & 1) ? (word >> 16) : (word & 0xFFFFu); }
__device__ __forceinline__ uint32_t half_count_bump(uint32_t *c, int kb) { return half_count_of(half_count_add(c, kb), kb); }
__device__ __forceinline__ void half_count_drop(uint32_t *c, int kb) { atomicSub(&c[kb >> 1], (kb & 1) ? 0x10000u : 1u); }
// the three path words an item of waypoint k needs: the waypoint, the one behind it (wn) and the one in front (wp), clamped to 0 .. lp
struct PathWords { uint32_t w, wn, wp; };
__device__ __forceinline__ PathWords path_words(const uint16_t *path, int k, int lp) {
    PathWords p;
    p.w = path[k]; p.wn = path[min(k + 1, lp)]; p.wp = path[max(k - 1, 0)];
    return p;
}
