// fl_obs_switches.h -- the diagnostic environment switches of the observation launcher: ONE table, a row a switch, read once per process.
// Host only: fl_obs.hip (the launcher) and fl_host.hip (fl_debug_obs_switches) include it, no header that the kernels include does.
// obs_switches() fills an ObsSwitches by a loop over the table at its first call -- every switch at once, where each used to be read when the
// launcher first came to it.  Every test and tool sets its switches in the environment of a fresh child process, so nothing depends on the difference.
#pragma once
#include <stdlib.h>
#include <string.h>

// FL_OBS_FORCE="nt=512,wl=8192,tab=0,nh=1,tmask=1,dual=0,items=0,snext=1": only configurations with these values (-1: any value)
struct ObsForce { int nt = -1, wl = -1, tab = -1, nh = -1, tmask = -1, dual = -1, items = -1, snext = -1; };
struct ObsSwitches {   // a long a row of the table, whatever its kind (a flag: 0 / 1) ...
    long verbose, no_fix, no_bins, no_split, no_wl_head, nt, lds_limit, tshift, forced, no_merge, round16, no_own_filter, no_fb, no_bk, no_compact,
         no_cutils_merge, no_cf_dirs, pb_ceil_split, no_early_topo, no_order, keep_verify;
    ObsForce force; bool bins_allowed, classes_allowed;   // ... the keys of FL_OBS_FORCE, and what follows from the table's `out` column: may a bin class / any launch class take the batch?
};

// a row's kind: how the variable's text becomes the field's value, `unset` where the variable does not exist
//   FLAG   1: the variable exists, whatever its value (empty and 0 count as set)
//   INT    atoi;  BYTES  atol
//   KEYS   1, and ObsSwitches::force: a key counts at the start of the string or right after a comma; unknown keys are ignored
enum ObsSwitchKind { OBS_SW_FLAG, OBS_SW_INT, OBS_SW_BYTES, OBS_SW_KEYS };
// what a row rules out.  A bin class REPLACES the batch's own options, so the switches that shape those options (what a same-box experiment wants
// to measure) rule the bins out; an exact class only ever matches options it dominates.  A switch that overrides what the classes' kernels have
// compiled in (threads, the LDS limit, the bucket width) rules out every launch class, split kernels included.
//   BINS         whenever the variable exists (FL_OBS_ROUND16=0 too)
//   CLASSES      when its value is not `unset`;  CLASSES_GE0  when its value is >= 0
enum ObsSwitchOut { OBS_OUT_NOTHING, OBS_OUT_BINS, OBS_OUT_CLASSES, OBS_OUT_CLASSES_GE0 };
struct ObsSwitchRow { const char *name; ObsSwitchKind kind; long ObsSwitches::*field; long unset; ObsSwitchOut out; const char *what; };
inline constexpr ObsSwitchRow OBS_SWITCH_TABLE[] = {
    {"FL_OBS_VERBOSE", OBS_SW_FLAG, &ObsSwitches::verbose, 0, OBS_OUT_NOTHING, "print the configuration obs_pick_config chose, for the first four launches"},
    {"FL_OBS_NO_FIX", OBS_SW_FLAG, &ObsSwitches::no_fix, 0, OBS_OUT_CLASSES, "the runtime carving for every batch"},
    {"FL_OBS_NO_BINS", OBS_SW_FLAG, &ObsSwitches::no_bins, 0, OBS_OUT_BINS, "exact classes only (the launcher of rounds 4 and 5)"},
    {"FL_OBS_NO_SPLIT", OBS_SW_FLAG, &ObsSwitches::no_split, 0, OBS_OUT_NOTHING, "no split kernels"},
    {"FL_OBS_NO_WL_HEAD", OBS_SW_FLAG, &ObsSwitches::no_wl_head, 0, OBS_OUT_NOTHING, "HBM work lists without their LDS head (rules out the classes that have one)"},
    {"FL_OBS_NT", OBS_SW_INT, &ObsSwitches::nt, 0, OBS_OUT_CLASSES, "only configurations of this many threads; 0: any (experiments on the LDS / occupancy trade-off)"},
    {"FL_OBS_LDS_LIMIT", OBS_SW_BYTES, &ObsSwitches::lds_limit, 160 * 1024, OBS_OUT_CLASSES, "the LDS a workgroup may take, in bytes (the same experiments)"},
    {"FL_OBS_TSHIFT", OBS_SW_INT, &ObsSwitches::tshift, -1, OBS_OUT_CLASSES_GE0, "time buckets of 1 << value steps; negative: the launcher's own"},
    {"FL_OBS_FORCE", OBS_SW_KEYS, &ObsSwitches::forced, 0, OBS_OUT_BINS, "only configurations with the listed option values"},
    {"FL_OBS_NO_MERGE", OBS_SW_FLAG, &ObsSwitches::no_merge, 0, OBS_OUT_BINS, "two stages instead of one pass B"},
    {"FL_OBS_ROUND16", OBS_SW_INT, &ObsSwitches::round16, -1, OBS_OUT_BINS, "rounds of 16 agents, two workgroups a CU -- 0: for no batch; 1: for envs of more than 32 agents; 2: for small envs too, whatever the batch"},
    {"FL_OBS_NO_OWN_FILTER", OBS_SW_FLAG, &ObsSwitches::no_own_filter, 0, OBS_OUT_BINS, "one-pass kernels: no own-path filter in the classify loop"},
    {"FL_OBS_NO_FB", OBS_SW_FLAG, &ObsSwitches::no_fb, 0, OBS_OUT_BINS, "one-pass kernels: plain lists, none grouped by time bucket"},
    {"FL_OBS_NO_BK", OBS_SW_FLAG, &ObsSwitches::no_bk, 0, OBS_OUT_BINS, "two-stage kernels: the flatland_cutils index not grouped by time bucket"},
    {"FL_OBS_NO_COMPACT", OBS_SW_FLAG, &ObsSwitches::no_compact, 0, OBS_OUT_NOTHING, "DFS-slot node tables for the upstream trees of every grid -- no depth 4"},
    {"FL_OBS_NO_CUTILS_MERGE", OBS_SW_FLAG, &ObsSwitches::no_cutils_merge, 0, OBS_OUT_NOTHING, "the builder alone on the stand-alone kernel, as before round 6"},
    {"FL_OBS_NO_CF_DIRS", OBS_SW_FLAG, &ObsSwitches::no_cf_dirs, 0, OBS_OUT_NOTHING, "classify loop: file every query, whatever the directions of the key's items"},
    {"FL_OBS_PB_CEIL_SPLIT", OBS_SW_FLAG, &ObsSwitches::pb_ceil_split, 0, OBS_OUT_NOTHING, "pass B: ceil(total / nt) cells a lane until none are left, as before the even slices"},
    {"FL_OBS_NO_EARLY_TOPO", OBS_SW_FLAG, &ObsSwitches::no_early_topo, 0, OBS_OUT_NOTHING, "one-round kernels: adjacency / padding rows / orders behind pass B, not beside its conflict scan"},
    {"FL_OBS_NO_ORDER", OBS_SW_FLAG, &ObsSwitches::no_order, 0, OBS_OUT_NOTHING, "workgroup k builds env k"},
    {"FL_OBS_KEEP_VERIFY", OBS_SW_FLAG, &ObsSwitches::keep_verify, 0, OBS_OUT_NOTHING, "check the keep-rows promise before every launch that skips the pre-fill (k_keep_verify)"},
};

inline void obs_force_read(ObsForce &f, const char *e) {
    const struct { const char *k; int *v; } keys[] = {{"nt=", &f.nt}, {"wl=", &f.wl}, {"tab=", &f.tab}, {"nh=", &f.nh}, {"tmask=", &f.tmask}, {"dual=", &f.dual}, {"items=", &f.items}, {"snext=", &f.snext}};
    for (const auto &kv : keys)
        if (const char *q = strstr(e, kv.k); q && (q == e || q[-1] == ',')) *kv.v = atoi(q + strlen(kv.k));
}
// the switches of this process: a reference to a static -- after the first call no look at the environment, no allocation, no string comparison
inline ObsSwitches obs_switches_read() {
    ObsSwitches s = {};
    s.bins_allowed = s.classes_allowed = true;
    for (const ObsSwitchRow &r : OBS_SWITCH_TABLE) {
        const char *e = getenv(r.name);
        const long v = s.*r.field = !e ? r.unset : r.kind == OBS_SW_INT ? atoi(e) : r.kind == OBS_SW_BYTES ? atol(e) : 1;
        if (e && r.kind == OBS_SW_KEYS) obs_force_read(s.force, e);
        if (e && r.out == OBS_OUT_BINS) s.bins_allowed = false;
        if (r.out == OBS_OUT_CLASSES ? v != r.unset : r.out == OBS_OUT_CLASSES_GE0 && v >= 0) s.classes_allowed = false;
    }
    return s;
}
inline const ObsSwitches &obs_switches() { static const ObsSwitches sw = obs_switches_read(); return sw; }
