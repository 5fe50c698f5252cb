// fl_obs_slices.h -- how pass B (wg_pass_b, fl_obs_passb.h) splits the `total` visited cells of a round of trees over the `nt` lanes of
// the workgroup: which cells a lane classifies, and the first and last cell of a wavefront.  Plain integer arithmetic without any other
// header, so that a host compiler takes this file alone (tests/test_passb_slices.py checks it for every total and block size).
//
// Even split: qlo = total / nt cells a lane and one more for the first rem = total % nt lanes -- the slices differ by at most one cell,
// the longer ones first, and every wavefront that can have a cell has one.  The split before it gave every lane ceil(total / nt) cells
// from lane 0 on until none were left: at cfg2 (3 180 cells on 1 024 lanes) that is four cells for 795 lanes and none for the last three
// wavefronts -- 16 / 12 / 12 / 12 wave-iterations on the four SIMDs where the even split has 13 / 13 / 12 / 12.  ceil_split keeps it
// for same-build comparisons (FL_OBS_PB_CEIL_SPLIT=1); it is the even rule with q = ceil(total / nt) and rem = 0, cut off at total.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FL_SLICE_FN __host__ __device__ inline
#else
#define FL_SLICE_FN inline
#endif

struct PbSplit {
    int q, rem, total;  // lane t starts at min(t * q + min(t, rem), total)
};

FL_SLICE_FN int pb_imin(int a, int b) { return a < b ? a : b; }

FL_SLICE_FN PbSplit pb_split(int total, int nt, bool ceil_split) {
    PbSplit s;
    s.q = (total + (ceil_split ? nt - 1 : 0)) / nt;
    s.rem = ceil_split ? 0 : total - s.q * nt;
    s.total = total;
    return s;
}
// lane t classifies the cells [pb_lane_begin, pb_lane_end) of the round (none: begin == end)
FL_SLICE_FN int pb_lane_begin(const PbSplit &s, int t) { return pb_imin(t * s.q + pb_imin(t, s.rem), s.total); }
FL_SLICE_FN int pb_lane_end(const PbSplit &s, int t) { return pb_lane_begin(s, t + 1); }
FL_SLICE_FN int pb_lane_cells(const PbSplit &s, int t) { return pb_lane_end(s, t) - pb_lane_begin(s, t); }
// wavefront w (lanes 64 w .. 64 w + 63): its first cell and its last; it has no cell when first == total (then last < first)
FL_SLICE_FN int pb_wave_first(const PbSplit &s, int w) { return pb_lane_begin(s, 64 * w); }
FL_SLICE_FN int pb_wave_last(const PbSplit &s, int w) { return pb_lane_begin(s, 64 * w + 64) - 1; }
// wavefronts of the workgroup without a cell
FL_SLICE_FN int pb_empty_waves(const PbSplit &s, int nt) {
    int n = 0;
    for (int w = 0; w < nt / 64; w++) n += pb_wave_first(s, w) >= s.total;
    return n;
}
