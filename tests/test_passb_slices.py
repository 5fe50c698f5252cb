"""CPU: the slice arithmetic of pass B (csrc/fl_obs_slices.h: which cells of a round a lane of k_obs classifies, the first and last cell of a
wavefront) checked exhaustively by a small stand-alone host program -- its own main, the header alone, no library -- for every total in
0 .. 6 000 and the block sizes 64, 256, 512, 1 024.  The GPU cannot be steered onto total % nt == 0 or a chosen remainder; this test carries
the arithmetic, tests/test_gpu_passb_slices.py the bytes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flatland_marl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include "fl_obs_slices.h"
#include <cstdio>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 20) std::printf("FAIL line %d: %s  (total %d nt %d lane/wave %d)\n", __LINE__, #c, total, nt, t); } } while (0)

// the split before the even slices, as wg_pass_b computed it: q = ceil(total / nt), pos = tid * q, end = min(pos + q, total)
static int old_q(int total, int nt) { return (total + nt - 1) / nt; }
static int old_pos(int total, int nt, int t) { return t * old_q(total, nt); }
static int old_end(int total, int nt, int t) { const int e = old_pos(total, nt, t) + old_q(total, nt); return e < total ? e : total; }

int main() {
    const int nts[4] = {64, 256, 512, 1024};
    long cases = 0;
    for (int k = 0; k < 4; k++) {
        const int nt = nts[k];
        for (int total = 0; total <= 6000; total++) {
            int t = -1;
            // ---- the even split
            const PbSplit s = pb_split(total, nt, false);
            const int qlo = total / nt, rem = total % nt;
            CHECK(s.q == qlo && s.rem == rem && s.total == total);
            CHECK(pb_lane_begin(s, 0) == 0);
            CHECK(pb_lane_end(s, nt - 1) == total);
            int longer = 0, prev_len = qlo + 1, empty_waves = 0;
            for (t = 0; t < nt; t++) {
                const int b = pb_lane_begin(s, t), e = pb_lane_end(s, t), len = e - b;
                CHECK(0 <= b && b <= e && e <= total);
                if (t + 1 < nt) CHECK(e == pb_lane_begin(s, t + 1));        // contiguous: with the two ends above, a partition of [0, total)
                CHECK(len == pb_lane_cells(s, t));
                CHECK(len == qlo || len == qlo + 1);                        // lengths differ by at most one ...
                CHECK(len <= prev_len);                                     // ... the longer ones first
                CHECK((len == qlo + 1) == (t < rem));
                prev_len = len;
                longer += len == qlo + 1;
                if (total <= nt) {                                          // at most a cell a lane: what the split before gave
                    CHECK(len == (t < total ? 1 : 0));
                    if (t < total) CHECK(b == old_pos(total, nt, t) && e == old_end(total, nt, t));
                }
            }
            t = -1;
            CHECK(longer == rem);
            if (rem == 0) CHECK(pb_lane_cells(s, 0) == qlo && pb_lane_cells(s, nt - 1) == qlo);
            if (total == 0) CHECK(pb_lane_begin(s, nt - 1) == 0 && pb_lane_end(s, 0) == 0);
            for (t = 0; t < nt / 64; t++) {                                 // (t: the wavefront)
                const int first = pb_wave_first(s, t), last = pb_wave_last(s, t);
                CHECK(first == pb_lane_begin(s, 64 * t));
                CHECK(last == pb_lane_end(s, 64 * t + 63) - 1);
                const bool has = pb_lane_cells(s, 64 * t) > 0;               // (no slice of a wavefront is longer than its first)
                CHECK(has == (first < total));
                CHECK(has == (last >= first));
                if (total >= nt) CHECK(has);                                 // a cell for every lane: no wavefront without
                empty_waves += !has;
            }
            t = -1;
            CHECK(empty_waves == pb_empty_waves(s, nt));
            // ---- FL_OBS_PB_CEIL_SPLIT: the same functions reproduce the split before, lane by lane and wavefront by wavefront
            const PbSplit c = pb_split(total, nt, true);
            CHECK(c.q == old_q(total, nt) && c.rem == 0);
            for (t = 0; t < nt; t++) {
                const int b = pb_lane_begin(c, t), e = pb_lane_end(c, t);
                const int ob = old_pos(total, nt, t), oe = old_end(total, nt, t);
                CHECK((b < e) == (ob < oe));
                if (ob < oe) CHECK(b == ob && e == oe);
                else CHECK(b == e);
            }
            for (t = 0; t < nt / 64; t++) {
                const int w0 = t * 64 * old_q(total, nt);
                CHECK((pb_wave_first(c, t) < total) == (w0 < total));
                if (w0 < total) {
                    const int wl = (w0 + 64 * old_q(total, nt) < total ? w0 + 64 * old_q(total, nt) : total) - 1;
                    CHECK(pb_wave_first(c, t) == w0 && pb_wave_last(c, t) == wl);
                }
            }
            cases++;
        }
    }
    // the headline's regime (about 3 180 cells on 1 024 lanes): the old split leaves three wavefronts without a cell, the even one none
    {
        const int total = 3180, nt = 1024, t = -1;
        CHECK(pb_empty_waves(pb_split(total, nt, true), nt) == 3);
        CHECK(pb_empty_waves(pb_split(total, nt, false), nt) == 0);
        CHECK(pb_lane_cells(pb_split(total, nt, false), 107) == 4 && pb_lane_cells(pb_split(total, nt, false), 108) == 3);
    }
    std::printf("%s %ld cases %d failures\n", fails ? "BAD" : "OK", cases, fails);
    return fails ? 1 : 0;
}
"""


def test_slices_partition_evenly_and_wavefront_ranges_match(tmp_path):
    src = tmp_path / "passb_slices_check.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "passb_slices_check")
    # host only: plain C++ (the header's functions are __host__ __device__ only under a HIP compile), no HIP runtime, no library of the project
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True, capture_output=True, text=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("0 failures") and run.stdout.strip().splitlines()[-1].startswith("OK 24004 cases"), run.stdout[-3000:]
