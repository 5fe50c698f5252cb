// fl_host.hip -- host side of the C-ABI (include/flatland_hip.h): device-resident SoA state, env hand-over,
// kernel launches on the handle's HIP stream.  No torch types; plain pointers and sizes.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/flatland_hip.h"
#include "fl_internal.h"
#include "fl_policy_layout.h"
#include "fl_static.h"
#include "fl_obs.h"
#include "fl_obs_switches.h"
#include "fl_global.h"
#include "fl_predict.h"
#include "fl_wrappers.h"
#include "../../include/flatland_predict.h"
#include "../../include/flatland_wrappers.h"

static thread_local char g_err[512] = "";
void fl_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
const char *fl_last_error(void) { return g_err; }
int fl_version(void) { return 100; }
int fl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

struct fl_batch {
    int device = 0;
    FlStatic s;  // host copy of every env's static description, the capacities, the owners of the shared tables (fl_static.h)
    FlDev d = {};
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::vector<void *> allocs;
    uint8_t *mask_dev = nullptr;   // [B] staging of host-side env masks (fl_reset, fl_commit after a live replacement)
    uint32_t *rcell_dev = nullptr; // [B][Rcap] cell id of a rail index (the copy of FlStatic::rcell; fl_predict turns waypoints back into cells)
    uint8_t *cellkind_dev = nullptr; // [B][H*W] bit 0 switch, bit 1 switch neighbour (k_decision_cells; the owners' slabs, as every static table)
    uint8_t *need_dev = nullptr;   // [B] the envs whose slabs a commit / full rebuild (re)builds: the OWNERS of shared static tables (FlDev::tab)
    FlObsScratch obs = {};
    int last_obs_launch[FL_OBS_LAUNCH_WORDS] = {-1};   // diagnostic: what the handle's last observation launch ran, written by the fl_launch_obs_* it calls (fl_debug_last_obs_launch); -1: none yet
};

template <typename T>
static int dev_alloc(fl_batch *h, T **p, size_t n) {
    HIPCHK(fl_alloc_zeroed(p, n, h->stream, h->allocs));
    return FL_OK;
}
#define DALLOC(ptr, n)                                   \
    do {                                                 \
        int rc_ = dev_alloc(h, &(ptr), (size_t)(n));     \
        if (rc_ != FL_OK) return rc_;                    \
    } while (0)

// free everything the handle allocated on the device; no device pointer is left behind
static void release_device(fl_batch *h) {
    for (void *p : h->allocs) (void)hipFree(p);
    h->allocs.clear();
    h->d = {};
    h->d.B = h->s.B; h->d.A = h->s.A; h->d.H = h->s.H; h->d.W = h->s.W;
    h->obs = {};
    h->mask_dev = nullptr; h->need_dev = nullptr;
    h->rcell_dev = nullptr; h->cellkind_dev = nullptr;
}

int fl_create(int B, int A, int H, int W, int device, fl_batch **out) {
    if (!out) { fl_set_error("fl_create: bad sizes"); return FL_ERR_ARG; }
    std::unique_ptr<fl_batch> h(new fl_batch());
    const int rc = fl_static_init(h->s, B, A, H, W);
    if (rc != FL_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fl_set_error("fl_create: no HIP device visible (the HIP path has no CPU fallback)");
        return FL_ERR_HIP;
    }
    HIPCHK(hipSetDevice(device));
    h->device = device;
    if (fl_step_lds_bytes(A) > 160 * 1024) {
        fl_set_error("fl_create: %d agents need %zu B of LDS per workgroup in the step kernel (limit 160 KiB)", A, fl_step_lds_bytes(A));
        return FL_ERR_ARG;
    }
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        fl_set_error("hipStreamCreate failed");
        return FL_ERR_HIP;
    }
    h->stream = h->own_stream;
    release_device(h.get());   // (nothing allocated yet: this sets FlDev to the batch sizes and no arrays)
    *out = h.release();
    return FL_OK;
}

void fl_destroy(fl_batch *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    release_device(h);
    (void)hipStreamDestroy(h->own_stream);
    delete h;
}

int fl_set_stream(fl_batch *h, void *hip_stream) {
    if (!h) return FL_ERR_ARG;
    h->stream = (hipStream_t)hip_stream;  // NULL = HIP's default (null) stream, which is what torch uses by default
    return FL_OK;
}

int fl_sync(fl_batch *h) {
    if (!h) return FL_ERR_ARG;
    HIPCHK(hipStreamSynchronize(h->stream));
    return FL_OK;
}

int fl_reserve(fl_batch *h, int max_targets, int max_rail_cells) {
    if (!h) { fl_set_error("fl_reserve: bad argument"); return FL_ERR_ARG; }
    // the reverse-BFS kernel keeps the env's neighbour table, four visited bitmaps and four queues in LDS (fl_dmap.hip)
    return fl_static_reserve(h->s, max_targets, max_rail_cells, [&](int rail_cells) {
        FlDev probe = h->d;
        probe.Rcap = rail_cells > 1 ? rail_cells : 1;
        probe.Ucap = 1;
        if (fl_dmap_fits(probe) == FL_OK) return true;
        fl_set_error("fl_reserve: %d rail cells per env do not fit the distance-map kernel's LDS", rail_cells);
        return false;
    });
}

int fl_load_env(fl_batch *h, int b, const uint16_t *grid, const int32_t *init_pos, const int32_t *init_dir,
                const int32_t *target, const double *speed, const int32_t *earliest, const int32_t *latest,
                int max_episode_steps, uint64_t malf_threshold, int malf_min, int malf_max, const uint32_t *mt_key,
                int mt_pos) {
    if (!h) { fl_set_error("fl_load_env: env index out of range"); return FL_ERR_ARG; }
    return fl_static_load(h->s, b, grid, init_pos, init_dir, target, speed, earliest, latest, max_episode_steps, malf_threshold, malf_min,
                          malf_max, mt_key, mt_pos);
}

// the device side of fl_static_arrays: allocate every array of the list ...
static int alloc_static_arrays(fl_batch *h) {
    return fl_static_arrays(h->s, h->d, h->rcell_dev, [&](const char *, auto &, auto *&dev, size_t per_env, int, bool present) {
        return present ? dev_alloc(h, &dev, (size_t)h->s.B * per_env) : (int)FL_OK;
    });
}
// ... and upload everything fl_load_env staged for envs [b0, b0 + nb): one copy per array
static int upload_envs(fl_batch *h, size_t b0, size_t nb) {
    return fl_static_arrays(h->s, h->d, h->rcell_dev, [&](const char *, auto &host, auto *&dev, size_t per_env, int, bool present) -> int {
        if (present) HIPCHK(hipMemcpyAsync(dev + b0 * per_env, host.data() + b0 * per_env, nb * per_env * sizeof *dev, hipMemcpyHostToDevice, h->stream));
        return FL_OK;
    });
}

// the chain of table kernels for the envs of mask_dev (u8[B]; through_tab: the OWNERS of the masked envs' tables, fl_launch_env_list)
static int launch_table_kernels(fl_batch *h, const uint8_t *mask_dev, bool through_tab) {
    fl_launch_env_list(h->d, mask_dev, h->stream, through_tab);
    HIPCHK(hipGetLastError());
    fl_launch_distance_maps(h->d, mask_dev, h->stream);
    HIPCHK(hipGetLastError());
    fl_launch_segments(h->d, mask_dev, h->stream);
    HIPCHK(hipGetLastError());
    fl_launch_nexthop(h->d, mask_dev, h->stream);
    HIPCHK(hipGetLastError());
    fl_launch_hop8(h->d, mask_dev, h->stream);
    HIPCHK(hipGetLastError());
    // the decision cells are a function of the rail grid alone: built for the owners a commit or a full rebuild names, not by a
    // masked rebuild (through_tab), which finds the grid -- and so this table -- as the last commit left it
    if (!through_tab) {
        fl_launch_decision_cells(h->d, mask_dev, h->cellkind_dev, h->stream);
        HIPCHK(hipGetLastError());
    }
    return FL_OK;
}

// the device side of the first commit: every device array of the handle, for the capacities the host side fixed
static int alloc_device(fl_batch *h) {
    // a first commit that failed half way (allocation, LDS fit) left device pointers behind: release them, a retry starts clean
    if (!h->allocs.empty()) release_device(h);
    FlDev &d = h->d;
    d.Ucap = h->s.Ucap; d.Rcap = h->s.Rcap;
    const size_t B = h->s.B, BA = B * h->s.A, HW = (size_t)h->s.H * h->s.W, Rcap = d.Rcap, Ucap = d.Ucap, Scap = Rcap * 4;
    {   // before anything is allocated: do the capacities fit the table kernels' LDS?
        const int rc_dm = fl_dmap_prepare(d);
        if (rc_dm != FL_OK) { fl_set_error("fl_commit: %d rail cells per env do not fit the distance-map kernel's LDS", d.Rcap); return rc_dm; }
    }
    int rc = alloc_static_arrays(h);
    if (rc != FL_OK) return rc;
    // the arrays that exist on the device only
    DALLOC(d.t, B); DALLOC(d.done_all, B);
    DALLOC(d.err, B); DALLOC(d.env_list, B + 1); DALLOC(d.metrics, B * 4); DALLOC(d.last_episode, B * 2); DALLOC(d.score_sums, B * 3);
    DALLOC(d.snext, B * Scap);
    DALLOC(d.dm, B * Ucap * Scap); DALLOC(d.seg, B * Scap);
    DALLOC(d.nh, B * Ucap * Rcap); DALLOC(d.hop8, B * Ucap * Scap);
    DALLOC(d.pos, BA); DALLOC(d.old_pos, BA); DALLOC(d.arrival, BA); DALLOC(d.malf, BA); DALLOC(d.pk, BA);
    DALLOC(h->mask_dev, B); DALLOC(h->need_dev, B); DALLOC(d.tab, B);
    DALLOC(h->cellkind_dev, B * HW);
    if (fl_step_prepare() != FL_OK) { fl_set_error("fl_commit: hipFuncSetAttribute failed"); return FL_ERR_HIP; }
    rc = fl_obs_alloc(h->obs, d, h->stream, h->allocs);
    if (rc != FL_OK) { fl_set_error("fl_commit: observation scratch allocation failed"); return rc; }
    return FL_OK;
}

int fl_commit(fl_batch *h) {
    if (!h) return FL_ERR_ARG;
    FlStatic &s = h->s;
    FlDev &d = h->d;
    const int B = s.B;
    const bool all = !s.committed;
    // the host side (fl_static.h): the capacities at the first commit, then the host tables of every env loaded since the last commit
    // and the owners of the shared tables.  Those envs are uploaded, the device tables of their owners rebuilt below, their agents reset (fresh)
    bool any = false;
    int rc = fl_static_commit_begin(s, &any);
    if (rc != FL_OK) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (all && (rc = alloc_device(h)) != FL_OK) return rc;
    h->obs.h_R = s.R.data();   // (host copy: which envs fit a fixed launch class, fl_obs.hip)
    d.max_branch = fl_static_max_branch(s);
    if (!any) return FL_OK;
    for (int b = 0; b < B;) {  // one set of copies per run of consecutive dirty envs (the first commit: one set in all)
        if (!s.dirty[b]) { b++; continue; }
        int e = b;
        while (e < B && s.dirty[e]) e++;
        rc = upload_envs(h, b, e - b);
        if (rc != FL_OK) return rc;
        b = e;
    }
    if (!all) HIPCHK(hipMemcpyAsync(h->mask_dev, s.dirty.data(), B, hipMemcpyHostToDevice, h->stream));
    const uint8_t *mask = all ? nullptr : h->mask_dev;
    // Shared static tables (FlDev::tab): envs with the same rail grid and the same unique targets read ONE set of tables, the
    // slabs of the first such env (the owner).  Built here: the owners whose slabs do not hold their content yet -- a new map, or
    // an env that becomes an owner because the previous one was replaced.
    HIPCHK(hipMemcpyAsync(d.tab, s.tab.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->need_dev, s.need.data(), B, hipMemcpyHostToDevice, h->stream));
    rc = launch_table_kernels(h, h->need_dev, false);
    if (rc != FL_OK) return rc;
    fl_launch_reset(d, mask, 1, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    fl_static_commit_end(s);
    return fl_check(h);
}

#define NEED_COMMIT(h)                                                         \
    do {                                                                       \
        if (!(h) || !(h)->s.committed) { fl_set_error("handle not committed"); return FL_ERR_ARG; } \
        HIPCHK(hipSetDevice((h)->device));                                     \
    } while (0)

// (the argument checks of an entry point that promises them before any HIP call)
#define NEED_COMMIT_NOHIP(h)                                                   \
    do {                                                                       \
        if (!(h) || !(h)->s.committed) { fl_set_error("handle not committed"); return FL_ERR_ARG; } \
    } while (0)

int fl_set_rng(fl_batch *h, const uint32_t *mt_key, const int32_t *mt_pos) {
    NEED_COMMIT(h);
    for (int b = 0; b < h->s.B; b++)
        if (mt_pos[b] < 0 || mt_pos[b] > 624) { fl_set_error("fl_set_rng: mt_pos out of range"); return FL_ERR_ARG; }
    HIPCHK(hipMemcpyAsync(h->d.mt, mt_key, (size_t)h->s.B * 624 * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d.mt_pos, mt_pos, (size_t)h->s.B * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return FL_OK;
}

int fl_get_rng(fl_batch *h, uint32_t *mt_key, int32_t *mt_pos) {
    NEED_COMMIT(h);
    HIPCHK(hipMemcpyAsync(mt_key, h->d.mt, (size_t)h->s.B * 624 * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(mt_pos, h->d.mt_pos, (size_t)h->s.B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return FL_OK;
}

int fl_reset(fl_batch *h, const uint8_t *mask, int fresh) {
    NEED_COMMIT(h);
    // the mask goes through a device buffer owned by the handle (no allocation, no host synchronisation here: a copy from
    // pageable memory returns once the source has been staged)
    if (mask) HIPCHK(hipMemcpyAsync(h->mask_dev, mask, h->s.B, hipMemcpyHostToDevice, h->stream));
    return fl_reset_dev(h, mask ? h->mask_dev : nullptr, fresh);
}

int fl_reset_dev(fl_batch *h, const uint8_t *mask_dev, int fresh) {
    NEED_COMMIT(h);
    // (the observation side keeps no state of its own across steps: the sticky deadlock flags live in the agents' packed word and
    // are cleared by k_reset -- flatland_cutils rebuilds its DeadlockChecker in TreeObsForRailEnv::reset(), treeobs.cpp:22-28)
    fl_launch_reset(h->d, mask_dev, fresh, h->stream);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_step(fl_batch *h, const uint8_t *actions_dev, int32_t *rewards_dev, uint8_t *dones_dev, uint8_t *done_all_dev,
            int auto_reset) {
    NEED_COMMIT(h);
    if (!actions_dev || !rewards_dev || !dones_dev || !done_all_dev) { fl_set_error("fl_step: null buffer"); return FL_ERR_ARG; }
    fl_launch_step(h->d, actions_dev, 0, 0, 0, rewards_dev, dones_dev, done_all_dev, auto_reset, h->stream);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_step_synth(fl_batch *h, uint32_t seed, uint32_t stream_base, int kind, int32_t *rewards_dev, uint8_t *dones_dev,
                  uint8_t *done_all_dev, int auto_reset) {
    NEED_COMMIT(h);
    if (!rewards_dev || !dones_dev || !done_all_dev || kind < 0 || kind > 2) { fl_set_error("fl_step_synth: bad argument"); return FL_ERR_ARG; }
    fl_launch_step(h->d, nullptr, seed, stream_base, kind, rewards_dev, dones_dev, done_all_dev, auto_reset, h->stream);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

// ---- the observation entry points (fl_step_obs, fl_obs_cutils, fl_obs_cutils_policy, fl_obs_cutils_handles, fl_obs_cutils_tree, fl_obs_tree,
// fl_obs_tree_handles) share one host path: obs_check_request, obs_handle_list for a handle list, then one of the obs_run_* below.  `who` is
// the entry point's name, the prefix of every message.
struct ObsTreeRequest {
    int min_depth, max_depth, pred_depth;
    double *out;
    bool compact_switch;   // refuse depth 4 under FL_OBS_NO_COMPACT here (the call launches something else before fl_launch_obs_tree would refuse it)
};
// Every argument check of an observation request, in the order all entry points have them: sizes, then pointers, then the depth-4 condition.
// c: the flatland_cutils part (with max_nodes and pred_depth; null: none), t: the upstream tree's (null: none; depth 0 where min_depth allows
// it: no tree in this call).  With both parts the tree's predicted path has to be a prefix of the cutils one.
static int obs_check_request(const fl_batch *h, const char *who, const FlObsCutilsOut *c, int max_nodes, int pred_depth, const ObsTreeRequest *t) {
    if (c && (max_nodes < 4 || max_nodes > FL_OBS_MAX_NODES || pred_depth < 1 || pred_depth > FL_OBS_MAX_PRED)) {
        fl_set_error("%s: max_nodes must be in [4,%d] and pred_depth in [1,%d]", who, FL_OBS_MAX_NODES, FL_OBS_MAX_PRED);
        return FL_ERR_ARG;
    }
    const bool tree = t && t->max_depth != 0;
    if (t) {
        const bool pred_ok = !tree || (c ? t->pred_depth >= 0 && t->pred_depth <= pred_depth : t->pred_depth <= FL_OBS_MAX_PRED);
        if (t->max_depth < t->min_depth || t->max_depth > FL_MAX_TREE_DEPTH || !pred_ok) {
            if (c) fl_set_error("%s: max_depth must be in [%d,%d] and 0 <= tree_pred_depth <= pred_depth", who, t->min_depth, FL_MAX_TREE_DEPTH);
            else fl_set_error("%s: max_depth must be in [%d,%d], pred_depth <= %d", who, t->min_depth, FL_MAX_TREE_DEPTH, FL_OBS_MAX_PRED);
            return FL_ERR_ARG;
        }
    }
    if ((c && (!c->attr || !c->forest || !c->adjacency || !c->node_order || !c->edge_order || !c->valid)) || (tree && !t->out)) {   // (props may be null)
        fl_set_error("%s: null output buffer", who);
        return FL_ERR_ARG;
    }
    // every argument error is raised BEFORE anything is launched: a depth-4 tree needs compact node tables (fl_launch_obs_tree's own check, which in
    // a call with a step or a cutils launch would fire after the envs have advanced a step and the cutils launch has set its sticky deadlock bits)
    if (tree && t->max_depth > 3 && (h->d.max_branch > 2 || (t->compact_switch && obs_switches().no_compact))) {
        fl_set_error("%s: max_depth 4 needs a grid on which no direction of a cell has more than two transitions (every Flatland rail cell type)%s; this batch has %d "
                "(nothing was launched: the envs have not advanced)", who, t->compact_switch ? " and the compact node tables" : "", h->d.max_branch);
        return FL_ERR_ARG;
    }
    return FL_OK;
}

// get_many(handles): the list has to be a permutation of 0 .. n_handles-1 (`reference`: what the reference builder does with any other list).
// *label_dev: the agents' list positions, staged on the device for the launch (FlObsScratch::label) -- null when the list is every agent in
// order, or when the call does not `use_list` (no predictor: no conflict test), which is the launch without a list.
static int obs_handle_list(fl_batch *h, const char *who, const int32_t *handles, int n_handles, const char *reference, bool use_list, const int16_t **label_dev) {
    const int A = h->s.A;
    *label_dev = nullptr;
    if (!handles || n_handles < 1 || n_handles > A) { fl_set_error("%s: 1 <= n_handles <= %d agents", who, A); return FL_ERR_ARG; }
    std::vector<int16_t> label(A, (int16_t)-1);
    bool identity = n_handles == A;
    for (int j = 0; j < n_handles; j++) {
        const int a = handles[j];
        if (a < 0 || a >= n_handles || label[a] >= 0) {
            fl_set_error("%s: handles has to be a permutation of 0 .. %d (handle %d at position %d): %s", who, n_handles - 1, a, j, reference);
            return FL_ERR_ARG;
        }
        label[a] = (int16_t)j;
        identity = identity && a == j;
    }
    if (identity || !use_list) return FL_OK;
    HIPCHK(hipMemcpyAsync(h->obs.label, label.data(), (size_t)A * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));      // (the staging vector is a local)
    *label_dev = h->obs.label;
    return FL_OK;
}

// the tail of every observation launch: rc is what the fl_launch_obs_* returned (it has written the handle's record, MODE -1 when nothing ran)
static int obs_launched(fl_batch *h, const char *who, int rc) {
    if (rc != FL_OK) {
        fl_set_error("%s: no launch configuration: %d rail cells and %d agents per env do not fit the observation kernels' LDS (160 KiB a workgroup), or the sizes are out of range", who, h->d.Rcap, h->d.A);
        return rc;
    }
    HIPCHK(hipGetLastError());
    return FL_OK;
}
// the launches of a checked request
static int obs_run_cutils(fl_batch *h, const char *who, int max_nodes, int pred_depth, const FlObsCutilsOut &out, const int16_t *label_dev = nullptr, int out64 = 0) {
    return obs_launched(h, who, fl_launch_obs_cutils(h->obs, h->d, max_nodes, pred_depth, out, h->stream, h->last_obs_launch, label_dev, out64));
}
static int obs_run_tree(fl_batch *h, const char *who, const ObsTreeRequest &t, const int16_t *label_dev = nullptr) {
    return obs_launched(h, who, fl_launch_obs_tree(h->obs, h->d, t.max_depth, t.pred_depth, t.out, h->stream, h->last_obs_launch, label_dev));
}
static int obs_run_both(fl_batch *h, const char *who, int max_nodes, int pred_depth, const FlObsCutilsOut &out, const ObsTreeRequest &t) {
    if (t.max_depth > 3 || max_nodes > 32) {   // beyond the fused kernels' node tables: the two builders one after the other (same outputs)
        const int rc = obs_run_cutils(h, who, max_nodes, pred_depth, out);
        return rc != FL_OK ? rc : obs_run_tree(h, who, t);
    }
    return obs_launched(h, who, fl_launch_obs_both(h->obs, h->d, max_nodes, pred_depth, out, t.max_depth, t.pred_depth, t.out, h->stream, h->last_obs_launch));
}

int fl_step_obs(fl_batch *h, const uint8_t *actions_dev, uint32_t seed, uint32_t stream_base, int kind, int32_t *rewards_dev,
                uint8_t *dones_dev, uint8_t *done_all_dev, int flags, int max_nodes, int pred_depth, float *attr_dev,
                float *forest_dev, int32_t *adjacency_dev, int32_t *node_order_dev, int32_t *edge_order_dev,
                uint8_t *valid_actions_dev, double *props_dev, int tree_max_depth, int tree_pred_depth, double *tree_out_dev) {
    NEED_COMMIT(h);
    if (!rewards_dev || !dones_dev || !done_all_dev || kind < 0 || kind > 2) { fl_set_error("fl_step_obs: bad step argument"); return FL_ERR_ARG; }
    const FlObsCutilsOut out = {attr_dev, forest_dev, adjacency_dev, node_order_dev, edge_order_dev, valid_actions_dev, props_dev};
    const ObsTreeRequest tree = {0, tree_max_depth, tree_pred_depth, tree_out_dev, true};
    const int rc = obs_check_request(h, "fl_step_obs", &out, max_nodes, pred_depth, &tree);
    if (rc != FL_OK) return rc;
    // TWO launches (k_step, then the observation kernel) back to back on the handle's stream behind this one call.  A single fused launch was
    // measured and is slower: the step wants one lane per agent and few wavefronts, the builders 16 wavefronts, and the second launch's dispatch overlaps the first.
    fl_launch_step(h->d, actions_dev, seed, stream_base, kind, rewards_dev, dones_dev, done_all_dev, flags, h->stream);
    HIPCHK(hipGetLastError());
    return tree_max_depth > 0 ? obs_run_both(h, "fl_step_obs", max_nodes, pred_depth, out, tree) : obs_run_cutils(h, "fl_step_obs", max_nodes, pred_depth, out);
}

int fl_check(fl_batch *h) {
    NEED_COMMIT(h);
    std::vector<int> err(h->s.B);
    HIPCHK(hipMemcpyAsync(err.data(), h->d.err, (size_t)h->s.B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int b = 0; b < h->s.B; b++) {
        if (err[b]) {
            const int e = err[b];
            HIPCHK(hipMemsetAsync(h->d.err, 0, (size_t)h->s.B * 4, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            const char *msg = e == FL_ERR_EPISODE_DONE ? "Episode is done, cannot call step()"
                              : e == FL_ERR_STATE_SYNC ? "agent state / position desync"
                              : e == FL_ERR_ZERO_TRANSITION ? "WRONG CELL TYPE detected in tree-search (0 transitions possible)"
                              : e == FL_ERR_CAPACITY ? "internal capacity exceeded"
                              : e == FL_ERR_ARG ? "FL_OBS_KEEP_TREE_ROWS: the tree buffer is not the previous launch's, or was modified in between (FL_OBS_KEEP_VERIFY)" : "kernel error";
            fl_set_error("env %d: %s", b, msg);
            return e;
        }
    }
    return FL_OK;
}

int fl_metrics(fl_batch *h, int64_t *out4_dev, int reset) {
    NEED_COMMIT(h);
    if (!out4_dev) { fl_set_error("fl_metrics: null buffer"); return FL_ERR_ARG; }
    fl_launch_metrics(h->d, (long long *)out4_dev, reset, h->stream);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_scores(fl_batch *h, double *out3_dev, int reset) {
    NEED_COMMIT(h);
    if (!out3_dev) { fl_set_error("fl_scores: null buffer"); return FL_ERR_ARG; }
    // (call it BEFORE fl_metrics(reset): the episode count it reports is fl_metrics' counter)
    fl_launch_scores(h->d, out3_dev, reset, h->stream);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_info(fl_batch *h, uint8_t *action_required_dev, int32_t *malfunction_dev, uint8_t *state_dev, double *scores_dev) {
    NEED_COMMIT(h);
    fl_launch_info(h->d, action_required_dev, malfunction_dev, state_dev, scores_dev, h->stream);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_policy_pack(int B, int A, int E, const int32_t *adjacency_dev, const int32_t *node_order_dev,
                   const int32_t *edge_order_dev, int64_t *adjacency_out_dev, int64_t *node_order_out_dev,
                   int64_t *edge_order_out_dev, void *hip_stream) {
    if (B <= 0 || A <= 0 || E <= 0 || !adjacency_dev || !node_order_dev || !edge_order_dev || !adjacency_out_dev ||
        !node_order_out_dev || !edge_order_out_dev) { fl_set_error("fl_policy_pack: bad argument"); return FL_ERR_ARG; }
    fl_launch_policy_pack(B, A, E, adjacency_dev, node_order_dev, edge_order_dev, (long long *)adjacency_out_dev,
                          (long long *)node_order_out_dev, (long long *)edge_order_out_dev, (hipStream_t)hip_stream);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_get_state(fl_batch *h, int32_t *state, int32_t *elapsed) {
    NEED_COMMIT(h);
    const size_t BA = (size_t)h->s.B * h->s.A;
    std::vector<int> pos(BA), old_pos(BA), arrival(BA);
    std::vector<uint32_t> malf(BA), pk(BA);
    HIPCHK(hipMemcpyAsync(pos.data(), h->d.pos, BA * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(old_pos.data(), h->d.old_pos, BA * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(arrival.data(), h->d.arrival, BA * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(malf.data(), h->d.malf, BA * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(pk.data(), h->d.pk, BA * 4, hipMemcpyDeviceToHost, h->stream));
    if (elapsed) HIPCHK(hipMemcpyAsync(elapsed, h->d.t, (size_t)h->s.B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int W = h->s.W;
    if (state) {
        for (size_t g = 0; g < BA; g++) {
            int32_t *o = state + g * FL_STATE_COLS;
            const uint32_t p = pk[g];
            o[0] = pos[g] < 0 ? -1 : pos[g] / W;
            o[1] = pos[g] < 0 ? -1 : pos[g] % W;
            o[2] = (int)PK_DIR(p);
            o[3] = (int)PK_STATE(p);
            o[4] = (int)(malf[g] & 0xFFFF);
            o[5] = (int)(malf[g] >> 16);
            o[6] = (int)PK_SCOUNT(p);
            o[7] = (int)PK_SAVED(p);
            o[8] = arrival[g];
            o[9] = old_pos[g] < 0 ? -1 : old_pos[g] / W;
            o[10] = old_pos[g] < 0 ? -1 : old_pos[g] % W;
            o[11] = PK_OLD_DIR(p) == 4 ? -1 : (int)PK_OLD_DIR(p);
        }
    }
    return FL_OK;
}

int fl_get_state_aux(fl_batch *h, int32_t *aux) {
    NEED_COMMIT(h);
    if (!aux) { fl_set_error("fl_get_state_aux: null buffer"); return FL_ERR_ARG; }
    const size_t BA = (size_t)h->s.B * h->s.A;
    std::vector<uint32_t> pk(BA);
    HIPCHK(hipMemcpyAsync(pk.data(), h->d.pk, BA * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t g = 0; g < BA; g++) {
        int32_t *o = aux + g * FL_AUX_COLS;
        o[0] = PK_PREV(pk[g]) == 7 ? -1 : (int)PK_PREV(pk[g]);
        o[1] = (int)PK_SIGMALF(pk[g]);
        o[2] = (int)PK_DEADLOCK(pk[g]);
        o[3] = (int)PK_DONE(pk[g]);
    }
    return FL_OK;
}

int fl_set_state(fl_batch *h, const int32_t *state, const int32_t *aux, const int32_t *elapsed, const uint8_t *done_all) {
    NEED_COMMIT(h);
    if (!state) { fl_set_error("fl_set_state: null state"); return FL_ERR_ARG; }
    const size_t BA = (size_t)h->s.B * h->s.A;
    const int H = h->s.H, W = h->s.W;
    std::vector<int> pos(BA), old_pos(BA), arrival(BA);
    std::vector<uint32_t> malf(BA), pk(BA);
    for (size_t g = 0; g < BA; g++) {
        const int32_t *o = state + g * FL_STATE_COLS;
        const int r = o[0], c = o[1], dir = o[2], st = o[3], mf = o[4], nmf = o[5], sc = o[6], sv = o[7], orow = o[9], ocol = o[10], od = o[11];
        const bool on = r >= 0;
        if ((on && (r >= H || c < 0 || c >= W)) || dir < 0 || dir > 3 || st < ST_WAITING || st > ST_DONE || mf < 0 || mf > 0xFFFF ||
            nmf < 0 || nmf > 0xFFFF || sc < 0 || sc > FL_MAX_SPEED_COUNT || sv < 0 || sv > 3 || od < -1 || od > 3 ||
            (orow >= 0 && (orow >= H || ocol < 0 || ocol >= W))) {
            fl_set_error("fl_set_state: env %zu agent %zu: value out of range", g / h->s.A, g % h->s.A);
            return FL_ERR_ARG;
        }
        // env_utils.state_position_sync_check (step_utils/env_utils.py:45-52)
        if ((st >= ST_MOVING && st <= ST_MALF && !on) || (st <= ST_MALF_OFF && on)) {
            fl_set_error("fl_set_state: env %zu agent %zu: state %d does not match position", g / h->s.A, g % h->s.A, st);
            return FL_ERR_STATE_SYNC;
        }
        pos[g] = on ? r * W + c : -1;
        old_pos[g] = orow >= 0 ? orow * W + ocol : -1;
        // an agent on the map stands on a rail cell: the kernels index the env's rail tables with the rail index of its position
        // (a cell without rail has none)
        const size_t hw0 = (g / h->s.A) * (size_t)H * W;
        if ((on && h->s.ridx[hw0 + pos[g]] == FL_R_NONE) || (orow >= 0 && h->s.ridx[hw0 + old_pos[g]] == FL_R_NONE)) {
            fl_set_error("fl_set_state: env %zu agent %zu: position (%d, %d) / old position (%d, %d) is not a rail cell", g / h->s.A, g % h->s.A, r, c, orow, ocol);
            return FL_ERR_STATE_SYNC;
        }
        arrival[g] = o[8];
        malf[g] = (uint32_t)mf | ((uint32_t)nmf << 16);
        int prev = 7, sig = mf > 0, dead = 0, done = st == ST_DONE;
        if (aux) {
            const int32_t *x = aux + g * FL_AUX_COLS;
            if (x[0] < -1 || x[0] > ST_DONE || (x[1] | x[2] | x[3]) < 0 || x[1] > 1 || x[2] > 1 || x[3] > 1) {
                fl_set_error("fl_set_state: env %zu agent %zu: aux value out of range", g / h->s.A, g % h->s.A);
                return FL_ERR_ARG;
            }
            prev = x[0] < 0 ? 7 : x[0]; sig = x[1]; dead = x[2]; done = x[3];
        }
        pk[g] = pk_make((uint32_t)dir, od < 0 ? 4u : (uint32_t)od, (uint32_t)st, (uint32_t)prev, (uint32_t)sv, (uint32_t)sc,
                        (uint32_t)sig, (uint32_t)dead, (uint32_t)done);
    }
    if (elapsed)
        for (int b = 0; b < h->s.B; b++)
            if (elapsed[b] < 0) { fl_set_error("fl_set_state: negative elapsed steps"); return FL_ERR_ARG; }
    HIPCHK(hipMemcpyAsync(h->d.pos, pos.data(), BA * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d.old_pos, old_pos.data(), BA * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d.arrival, arrival.data(), BA * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d.malf, malf.data(), BA * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d.pk, pk.data(), BA * 4, hipMemcpyHostToDevice, h->stream));
    if (elapsed) HIPCHK(hipMemcpyAsync(h->d.t, elapsed, (size_t)h->s.B * 4, hipMemcpyHostToDevice, h->stream));
    if (done_all) HIPCHK(hipMemcpyAsync(h->d.done_all, done_all, (size_t)h->s.B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // the staging vectors are locals
    return FL_OK;
}

int fl_motion_check(int device, int n_cases, const int32_t *offsets, const int32_t *cur, const int32_t *nxt, uint8_t *can_move) {
    if (n_cases <= 0 || !offsets || !cur || !nxt || !can_move) { fl_set_error("fl_motion_check: bad argument"); return FL_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fl_set_error("fl_motion_check: no HIP device visible"); return FL_ERR_HIP; }
    int max_agents = 0;
    for (int c = 0; c < n_cases; c++) {
        const int n = offsets[c + 1] - offsets[c];
        if (n < 0 || n > 1024) { fl_set_error("fl_motion_check: case %d has %d agents (0..1024 supported)", c, n); return FL_ERR_ARG; }
        max_agents = n > max_agents ? n : max_agents;
    }
    const int total = offsets[n_cases] - offsets[0];
    for (int k = offsets[0]; k < offsets[n_cases]; k++)
        if (cur[k] < -1 || nxt[k] < -1 || cur[k] >= (1 << 28) || nxt[k] >= (1 << 28)) { fl_set_error("fl_motion_check: cell id out of range"); return FL_ERR_ARG; }
    if (offsets[0] != 0) { fl_set_error("fl_motion_check: offsets must start at 0"); return FL_ERR_ARG; }
    HIPCHK(hipSetDevice(device));
    int *d_off = nullptr, *d_cur = nullptr, *d_nxt = nullptr;
    uint8_t *d_out = nullptr;
    const size_t nb = (size_t)(total > 0 ? total : 1);
    hipError_t e = hipMalloc((void **)&d_off, (size_t)(n_cases + 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_cur, nb * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_nxt, nb * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, nb);
    if (e == hipSuccess) e = hipMemcpy(d_off, offsets, (size_t)(n_cases + 1) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && total > 0) e = hipMemcpy(d_cur, cur, nb * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && total > 0) e = hipMemcpy(d_nxt, nxt, nb * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        fl_launch_motion_check(n_cases, max_agents, d_off, d_cur, d_nxt, d_out, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && total > 0) e = hipMemcpy(can_move, d_out, nb, hipMemcpyDeviceToHost);
    (void)hipFree(d_off); (void)hipFree(d_cur); (void)hipFree(d_nxt); (void)hipFree(d_out);
    if (e != hipSuccess) { fl_set_error("fl_motion_check: %s", hipGetErrorString(e)); return FL_ERR_HIP; }
    return FL_OK;
}

int fl_distance_map(fl_batch *h, int b, int *n_targets, uint16_t *dm, int32_t *target_slot) {
    NEED_COMMIT(h);
    if (b < 0 || b >= h->s.B || !n_targets) { fl_set_error("fl_distance_map: bad argument"); return FL_ERR_ARG; }
    const int U = h->s.U[b], R = h->s.R[b];
    *n_targets = U;
    const size_t HW = (size_t)h->s.H * h->s.W, Scap = (size_t)h->d.Rcap * 4;
    if (target_slot) memcpy(target_slot, &h->s.tslot[(size_t)b * h->s.A], (size_t)h->s.A * 4);
    if (dm) {  // the resident map holds rail states only: expand it to the reference's dense [U][H][W][4]
        std::vector<uint16_t> rs((size_t)U * Scap);
        HIPCHK(hipMemcpyAsync(rs.data(), h->d.dm + (size_t)h->s.tab[b] * h->d.Ucap * Scap, rs.size() * 2, hipMemcpyDeviceToHost, h->stream));   // (the owner's slab)
        HIPCHK(hipStreamSynchronize(h->stream));
        const uint32_t *rcell = &h->s.rcell[(size_t)b * h->d.Rcap];
        for (size_t k = 0; k < (size_t)U * HW * 4; k++) dm[k] = FL_INF16;
        for (int u = 0; u < U; u++)
            for (int r = 0; r < R; r++)
                memcpy(&dm[((size_t)u * HW + rcell[r]) * 4], &rs[(size_t)u * Scap + (size_t)r * 4], 8);
    }
    return FL_OK;
}

static int rebuild_tables(fl_batch *h, const uint8_t *mask_dev) {
    // every env: each OWNER once (host mask); a device mask of envs: the owners of the masked envs (FlDev::tab), an owner once per
    // masked env that reads it -- DistanceMap.reset() + _compute() of every env that resets, as the reference does it
    if (!mask_dev) {
        for (int b = 0; b < h->s.B; b++) h->s.need[b] = h->s.tab[b] == b;
        HIPCHK(hipMemcpyAsync(h->need_dev, h->s.need.data(), h->s.B, hipMemcpyHostToDevice, h->stream));
    }
    return launch_table_kernels(h, mask_dev ? mask_dev : h->need_dev, mask_dev != nullptr);
}

int fl_distance_map_rebuild(fl_batch *h) {
    NEED_COMMIT(h);
    return rebuild_tables(h, nullptr);
}

int fl_distance_map_rebuild_masked(fl_batch *h, const uint8_t *mask_dev) {
    NEED_COMMIT(h);
    if (!mask_dev) { fl_set_error("fl_distance_map_rebuild_masked: null mask"); return FL_ERR_ARG; }
    return rebuild_tables(h, mask_dev);
}

int fl_positions_map(fl_batch *h, int b, int32_t *out) {
    NEED_COMMIT(h);
    if (b < 0 || b >= h->s.B || !out) { fl_set_error("fl_positions_map: bad argument"); return FL_ERR_ARG; }
    // RailEnv._update_agent_positions_map (rail_env.py:360-367): later agents overwrite earlier ones on a shared cell
    const int A = h->s.A;
    std::vector<int> pos(A);
    HIPCHK(hipMemcpyAsync(pos.data(), h->d.pos + (size_t)b * A, (size_t)A * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t c = 0; c < (size_t)h->s.H * h->s.W; c++) out[c] = -1;
    for (int i = 0; i < A; i++)
        if (pos[i] >= 0) out[pos[i]] = i;
    return FL_OK;
}

int fl_obs_cutils(fl_batch *h, int max_nodes, int pred_depth, float *attr_dev, float *forest_dev, int32_t *adjacency_dev,
                  int32_t *node_order_dev, int32_t *edge_order_dev, uint8_t *valid_actions_dev, double *props_dev) {
    NEED_COMMIT(h);
    const FlObsCutilsOut out = {attr_dev, forest_dev, adjacency_dev, node_order_dev, edge_order_dev, valid_actions_dev, props_dev};
    const int rc = obs_check_request(h, "fl_obs_cutils", &out, max_nodes, pred_depth, nullptr);
    return rc != FL_OK ? rc : obs_run_cutils(h, "fl_obs_cutils", max_nodes, pred_depth, out);
}

int fl_obs_cutils_policy(fl_batch *h, int max_nodes, int pred_depth, float *attr_dev, float *forest_dev, int64_t *adjacency_dev,
                         int64_t *node_order_dev, int64_t *edge_order_dev, uint8_t *valid_actions_dev, double *props_dev) {
    NEED_COMMIT(h);
    const FlObsCutilsOut out = {attr_dev, forest_dev, reinterpret_cast<int32_t *>(adjacency_dev), reinterpret_cast<int32_t *>(node_order_dev),
                                reinterpret_cast<int32_t *>(edge_order_dev), valid_actions_dev, props_dev};
    const int rc = obs_check_request(h, "fl_obs_cutils_policy", &out, max_nodes, pred_depth, nullptr);
    return rc != FL_OK ? rc : obs_run_cutils(h, "fl_obs_cutils_policy", max_nodes, pred_depth, out, nullptr, 1);
}

int fl_obs_cutils_handles(fl_batch *h, int max_nodes, int pred_depth, const int32_t *handles, int n_handles, float *attr_dev,
                          float *forest_dev, int32_t *adjacency_dev, int32_t *node_order_dev, int32_t *edge_order_dev,
                          uint8_t *valid_actions_dev, double *props_dev) {
    NEED_COMMIT(h);
    // the reference's conflict test erases position `agent.handle` from a list of len(handles) entries (tool.h:428-434): a listed
    // handle >= len(handles) is undefined behaviour there; what remains are the permutations of 0 .. n-1
    const int16_t *label_dev;
    int rc = obs_handle_list(h, "fl_obs_cutils_handles", handles, n_handles, "the reference's get_many is undefined for any other strict subset "
                             "(treeobs.cpp:393-401 erases list position `handle`)", true, &label_dev);
    if (rc != FL_OK) return rc;
    const FlObsCutilsOut out = {attr_dev, forest_dev, adjacency_dev, node_order_dev, edge_order_dev, valid_actions_dev, props_dev};
    rc = obs_check_request(h, "fl_obs_cutils_handles", &out, max_nodes, pred_depth, nullptr);
    return rc != FL_OK ? rc : obs_run_cutils(h, "fl_obs_cutils_handles", max_nodes, pred_depth, out, label_dev);
}

int fl_obs_cutils_tree(fl_batch *h, int max_nodes, int pred_depth, float *attr_dev, float *forest_dev, int32_t *adjacency_dev,
                       int32_t *node_order_dev, int32_t *edge_order_dev, uint8_t *valid_actions_dev, double *props_dev,
                       int tree_max_depth, int tree_pred_depth, double *tree_out_dev) {
    NEED_COMMIT(h);
    const FlObsCutilsOut out = {attr_dev, forest_dev, adjacency_dev, node_order_dev, edge_order_dev, valid_actions_dev, props_dev};
    const ObsTreeRequest tree = {1, tree_max_depth, tree_pred_depth, tree_out_dev, true};   // (depth 4: before the cutils launch sets its sticky deadlock bits)
    const int rc = obs_check_request(h, "fl_obs_cutils_tree", &out, max_nodes, pred_depth, &tree);
    return rc != FL_OK ? rc : obs_run_both(h, "fl_obs_cutils_tree", max_nodes, pred_depth, out, tree);
}

int fl_obs_global(fl_batch *h, int b0, int nb, int elem_bytes, void *rail_dev, void *agents_state_dev, void *targets_dev) {
    NEED_COMMIT(h);
    if (b0 < 0 || nb < 1 || b0 > h->s.B - nb) { fl_set_error("fl_obs_global: env range [%d, %d + %d) is not inside [0, %d)", b0, b0, nb, h->s.B); return FL_ERR_ARG; }
    if (elem_bytes != 4 && elem_bytes != 8) { fl_set_error("fl_obs_global: elem_bytes must be 8 (float64) or 4 (float32), got %d", elem_bytes); return FL_ERR_ARG; }
    if (!rail_dev && !agents_state_dev && !targets_dev) { fl_set_error("fl_obs_global: every output buffer is NULL"); return FL_ERR_ARG; }
    if (((uintptr_t)rail_dev | (uintptr_t)agents_state_dev | (uintptr_t)targets_dev) & 15u) {
        fl_set_error("fl_obs_global: the output buffers must be 16-byte aligned");
        return FL_ERR_ARG;
    }
    if (fl_launch_obs_global(h->d, b0, nb, elem_bytes, h->obs.n_cu, rail_dev, agents_state_dev, targets_dev, h->stream) != FL_OK) {
        fl_set_error("fl_obs_global: a %d x %d map needs more bands of cells than one launch holds", h->s.H, h->s.W);
        return FL_ERR_ARG;
    }
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_predict(fl_batch *h, int b0, int nb, int max_depth, int elem_kind, void *pred_dev, int32_t *path_dev, int32_t *path_len_dev) {
    NEED_COMMIT_NOHIP(h);
    if (b0 < 0 || nb < 1 || b0 > h->s.B - nb) { fl_set_error("fl_predict: env range [%d, %d + %d) is not inside [0, %d)", b0, b0, nb, h->s.B); return FL_ERR_ARG; }
    if (max_depth < 1 || max_depth > FLP_MAX_DEPTH) { fl_set_error("fl_predict: max_depth must be in 1 .. %d, got %d", FLP_MAX_DEPTH, max_depth); return FL_ERR_ARG; }
    if (elem_kind != 0 && elem_kind != 1) { fl_set_error("fl_predict: elem_kind must be 0 (float64) or 1 (int32), got %d", elem_kind); return FL_ERR_ARG; }
    if (!pred_dev && !path_dev && !path_len_dev) { fl_set_error("fl_predict: every output buffer is NULL"); return FL_ERR_ARG; }
    if ((path_dev == nullptr) != (path_len_dev == nullptr)) { fl_set_error("fl_predict: path_dev and path_len_dev go together"); return FL_ERR_ARG; }
    if ((uintptr_t)pred_dev & 15u) { fl_set_error("fl_predict: pred_dev must be 16-byte aligned"); return FL_ERR_ARG; }
    HIPCHK(hipSetDevice(h->device));
    if (fl_launch_predict(h->d, h->rcell_dev, b0, nb, max_depth, elem_kind, h->obs.n_cu, pred_dev, path_dev, path_len_dev, h->stream) != FL_OK) {
        fl_set_error("fl_predict: %d envs of %d agents are more workgroups than one launch holds", nb, h->s.A);
        return FL_ERR_ARG;
    }
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_action_space(fl_batch *h, int b0, int nb, int elem_kind, uint8_t *sp_action_dev, void *sp_dist_dev, uint8_t *sp_count_dev,
                    uint8_t *on_decision_dev, const uint8_t *reduced_dev, uint8_t *actions_dev) {
    NEED_COMMIT_NOHIP(h);
    if (b0 < 0 || nb < 1 || b0 > h->s.B - nb) { fl_set_error("fl_action_space: env range [%d, %d + %d) is not inside [0, %d)", b0, b0, nb, h->s.B); return FL_ERR_ARG; }
    if (elem_kind != 0 && elem_kind != 1) { fl_set_error("fl_action_space: elem_kind must be 0 (float64) or 1 (int32), got %d", elem_kind); return FL_ERR_ARG; }
    if (!sp_action_dev && !sp_dist_dev && !sp_count_dev && !on_decision_dev && !actions_dev && !reduced_dev) { fl_set_error("fl_action_space: every output buffer is NULL"); return FL_ERR_ARG; }
    if ((sp_action_dev == nullptr) != (sp_dist_dev == nullptr) || (sp_action_dev == nullptr) != (sp_count_dev == nullptr)) {
        fl_set_error("fl_action_space: sp_action_dev, sp_dist_dev and sp_count_dev go together");
        return FL_ERR_ARG;
    }
    if ((reduced_dev == nullptr) != (actions_dev == nullptr)) { fl_set_error("fl_action_space: reduced_dev and actions_dev go together"); return FL_ERR_ARG; }
    if ((uintptr_t)sp_dist_dev & (elem_kind == 0 ? 7u : 3u)) { fl_set_error("fl_action_space: sp_dist_dev must be %d-byte aligned", elem_kind == 0 ? 8 : 4); return FL_ERR_ARG; }
    HIPCHK(hipSetDevice(h->device));
    if (fl_launch_action_space(h->d, h->cellkind_dev, b0, nb, elem_kind, h->obs.n_cu, sp_action_dev, sp_dist_dev, sp_count_dev, on_decision_dev, reduced_dev,
                               actions_dev, h->stream) != FL_OK) {
        fl_set_error("fl_action_space: %d envs of %d agents are more workgroups than one launch holds", nb, h->s.A);
        return FL_ERR_ARG;
    }
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_decision_cells(fl_batch *h, int b0, int nb, uint8_t *cells_dev) {
    NEED_COMMIT_NOHIP(h);
    if (b0 < 0 || nb < 1 || b0 > h->s.B - nb) { fl_set_error("fl_decision_cells: env range [%d, %d + %d) is not inside [0, %d)", b0, b0, nb, h->s.B); return FL_ERR_ARG; }
    if (!cells_dev) { fl_set_error("fl_decision_cells: cells_dev is NULL"); return FL_ERR_ARG; }
    HIPCHK(hipSetDevice(h->device));
    fl_launch_decision_cells_out(h->d, h->cellkind_dev, b0, nb, cells_dev, h->stream);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_obs_set_mode(fl_batch *h, int flags) {
    NEED_COMMIT(h);
    if (flags & ~FL_OBS_KEEP_TREE_ROWS) { fl_set_error("fl_obs_set_mode: unknown flag"); return FL_ERR_ARG; }
    h->obs.keep_rows = (flags & FL_OBS_KEEP_TREE_ROWS) != 0;
    h->obs.rows_out = nullptr;      // the next launch fills its whole slab and starts the row masks afresh
    return FL_OK;
}

int fl_obs_tree(fl_batch *h, int max_depth, int pred_depth, double *out_dev) {
    NEED_COMMIT(h);
    const ObsTreeRequest tree = {1, max_depth, pred_depth, out_dev, false};
    const int rc = obs_check_request(h, "fl_obs_tree", nullptr, 0, 0, &tree);
    return rc != FL_OK ? rc : obs_run_tree(h, "fl_obs_tree", tree);
}

int fl_obs_tree_handles(fl_batch *h, int max_depth, int pred_depth, const int32_t *handles, int n_handles, double *out_dev) {
    NEED_COMMIT(h);
    // the reference's conflict test deletes position `handle` from the arrays of the listed handles' predictions and reads
    // env.agents[position].state (observations.py:337-366): a listed handle >= len(handles) is an IndexError there; what remains are
    // the permutations of 0 .. n-1
    const int16_t *label_dev;
    int rc = obs_handle_list(h, "fl_obs_tree_handles", handles, n_handles, "the reference's get_many raises IndexError for a handle >= len(handles) "
                             "(observations.py:337 deletes list position `handle`)", pred_depth >= 0, &label_dev);   // (no predictor: no conflict test, the list does not matter)
    if (rc != FL_OK) return rc;
    const ObsTreeRequest tree = {1, max_depth, pred_depth, out_dev, false};
    rc = obs_check_request(h, "fl_obs_tree_handles", nullptr, 0, 0, &tree);
    return rc != FL_OK ? rc : obs_run_tree(h, "fl_obs_tree_handles", tree, label_dev);
}

// diagnostic (not part of the public header): copy the per-env phase clocks of a -DFL_OBS_TIMING build
extern "C" int fl_debug_obs_clocks(fl_batch *h, long long *out /* [B][64] */) {
    NEED_COMMIT(h);
    HIPCHK(hipMemcpyAsync(out, h->obs.dbg, (size_t)h->s.B * 64 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return FL_OK;
}

// diagnostic (not part of the public header): threads, LDS bytes, keys in LDS, next-hop in LDS, work-list bytes, time masks,
// second index, items in LDS, one pass B for both builders, compact upstream trees of the fused observation launch on this batch
extern "C" int fl_debug_obs_config(fl_batch *h, int pred_depth, int max_depth, int tree_pred, int *out11) {
    NEED_COMMIT(h);
    return fl_obs_config_of_fused(h->d, pred_depth, max_depth, tree_pred, out11, obs_batch_is_wide(h->d.B, h->obs.n_cu));
}

// diagnostic (not part of the public header), no GPU needed: does the launcher take a batch of B small envs on n_cu CUs as two workgroups a CU
extern "C" int fl_debug_batch_is_wide(int B, int n_cu) { return obs_batch_is_wide(B, n_cu) ? 1 : 0; }

// diagnostic (not part of the public header): what the last fused observation launch (fl_obs_cutils_tree / fl_step_obs with a tree)
// of this handle ran -- out[0] fixed launch class (0 = the runtime-carving kernel), out[1] 1 = the class's split kernel (the class's
// body only for the envs that fit it), out[2] envs that took the class's body
extern "C" int fl_debug_last_obs_class(fl_batch *h, int *out3) {
    if (!h || !out3) return FL_ERR_ARG;
    out3[0] = h->obs.last_fix; out3[1] = h->obs.last_split; out3[2] = h->obs.last_fit;
    return FL_OK;
}

// diagnostic (not part of the public header): what the handle's last observation launch ran, through any of fl_obs_cutils*, fl_obs_tree*, fl_obs_cutils_tree and
// fl_step_obs -- FL_OBS_LAUNCH_WORDS ints as fl_obs.h lists them (kernel MODE / VAR / class / split, threads, LDS bytes, the accepted options, what the launcher
// derived from them); MODE -1: no launch yet, or the last call found no configuration
extern "C" int fl_debug_last_obs_launch(fl_batch *h, int *out, int n_out) {
    if (!h || !out || n_out < FL_OBS_LAUNCH_WORDS) return FL_ERR_ARG;
    memcpy(out, h->last_obs_launch, sizeof h->last_obs_launch);
    return FL_OK;
}

// diagnostic (not part of the public header), no GPU needed: the same for a batch of the given sizes -- agents, rail-cell and
// unique-target capacities, maps taller than wide (compact prediction keys), most transitions of a (cell, direction)
static int obs_config_of(int A, int Rcap, int Ucap, int tall, int max_branch, int pred_depth, int max_depth, int tree_pred, int *out11, int wide) {
    FlDev d;
    memset(&d, 0, sizeof d);
    d.A = A; d.Rcap = Rcap; d.Ucap = Ucap; d.max_branch = max_branch;
    static uint16_t dummy_key;
    d.rkey = tall ? &dummy_key : nullptr;
    return fl_obs_config_of_fused(d, pred_depth, max_depth, tree_pred, out11, wide);
}
extern "C" int fl_debug_obs_config_of(int A, int Rcap, int Ucap, int tall, int max_branch, int pred_depth, int max_depth, int tree_pred,
                                      int *out11) {
    return obs_config_of(A, Rcap, Ucap, tall, max_branch, pred_depth, max_depth, tree_pred, out11, 0);
}
// ... of a WIDE batch (several envs per CU)
extern "C" int fl_debug_obs_config_of_wide(int A, int Rcap, int Ucap, int tall, int max_branch, int pred_depth, int max_depth, int tree_pred,
                                           int *out11) {
    return obs_config_of(A, Rcap, Ucap, tall, max_branch, pred_depth, max_depth, tree_pred, out11, 1);
}
// diagnostic (not part of the public header), no GPU needed: the whole launch plan of fl_obs_cutils* (kind 0), fl_obs_cutils_tree / fl_step_obs
// with a tree (1) or fl_obs_tree* (2) on a device of n_cu CUs for a batch of B envs with R[b] rail cells each -- the host path of the launch up
// to the enqueue (its limits, arguments, the preference walk, the launch class, the split class), so also what fl_debug_obs_config_of cannot
// see: split launches, FL_OBS_KEEP_TREE_ROWS (keep_mode 1) and a handle subset (label 1).  record: the FL_OBS_LAUNCH_WORDS ints that
// fl_debug_last_obs_launch would report after the launch; *n_fit: the envs on the launch class's body.  FL_ERR_ARG where the launch returns it.
extern "C" int fl_debug_obs_plan(int kind, int A, int Ucap, int tall, int max_branch, int max_nodes, int pred_depth, int max_depth, int tree_pred,
                                 int keep_mode, int label, int n_cu, const int *R, int B, int *record, int *n_fit) {
    if (!R || B <= 0 || !record || !n_fit) return FL_ERR_ARG;
    FlDev d;
    memset(&d, 0, sizeof d);
    d.B = B; d.A = A; d.Rcap = *std::max_element(R, R + B); d.Ucap = Ucap; d.max_branch = max_branch;
    static uint16_t dummy_key;
    static int16_t dummy_label;
    d.rkey = tall ? &dummy_key : nullptr;
    FlObsScratch o;
    memset(&o, 0, sizeof o);
    o.pred_cap = FL_OBS_MAX_PRED + 2; o.n_cu = n_cu; o.h_R = R; o.keep_rows = keep_mode;
    *n_fit = 0;
    return fl_obs_plan(kind, o, d, max_nodes, pred_depth, max_depth, tree_pred, label ? &dummy_label : nullptr, record, n_fit);
}

// diagnostic (not part of the public header), no GPU needed: the launcher's table of environment switches (fl_obs_switches.h), a line a switch --
// "NAME kind rules-out\n", kind flag / int / bytes / keys, rules-out nothing / bins / classes.  Returns the bytes of it with the final 0
// (written when they fit `cap`).
extern "C" int fl_debug_obs_switches(char *out, int cap) {
    static const char *const kinds[] = {"flag", "int", "bytes", "keys"}, *const outs[] = {"nothing", "bins", "classes", "classes"};
    int n = 1;
    for (const ObsSwitchRow &r : OBS_SWITCH_TABLE) n += snprintf(nullptr, 0, "%s %s %s\n", r.name, kinds[r.kind], outs[r.out]);
    if (!out || n > cap) return n;
    for (const ObsSwitchRow &r : OBS_SWITCH_TABLE) out += sprintf(out, "%s %s %s\n", r.name, kinds[r.kind], outs[r.out]);
    return n;
}

// diagnostic (not part of the public header), no GPU needed: the host half of a handle alone -- an FlStatic (fl_static.h) behind an opaque
// pointer, driven by the functions fl_create / fl_load_env / fl_reserve / fl_commit call for theirs (same codes, same messages).
extern "C" FlStatic *fl_debug_static_new(int B, int A, int H, int W) {   // null: fl_create's refusal of the sizes
    std::unique_ptr<FlStatic> s(new FlStatic());
    return fl_static_init(*s, B, A, H, W) == FL_OK ? s.release() : nullptr;
}
extern "C" void fl_debug_static_free(FlStatic *s) { delete s; }
extern "C" int fl_debug_static_load(FlStatic *s, int b, const uint16_t *grid, const int32_t *init_pos, const int32_t *init_dir, const int32_t *target,
                                    const double *speed, const int32_t *earliest, const int32_t *latest, int max_episode_steps,
                                    uint64_t malf_threshold, int malf_min, int malf_max, const uint32_t *mt_key, int mt_pos) {
    if (!s) return FL_ERR_ARG;
    return fl_static_load(*s, b, grid, init_pos, init_dir, target, speed, earliest, latest, max_episode_steps, malf_threshold, malf_min, malf_max,
                          mt_key, mt_pos);
}
extern "C" int fl_debug_static_reserve(FlStatic *s, int max_targets, int max_rail_cells) {   // (without the distance-map kernel's LDS limit)
    return s ? fl_static_reserve(*s, max_targets, max_rail_cells, [](int) { return true; }) : (int)FL_ERR_ARG;
}
extern "C" int fl_debug_static_commit(FlStatic *s) {
    if (!s) return FL_ERR_ARG;
    bool any = false;
    const int rc = fl_static_commit_begin(*s, &any);
    if (rc == FL_OK && any) fl_static_commit_end(*s);
    return rc;
}
// copy out array `name` -- of fl_static_arrays, or grid / ut / maxbr / loaded / dirty / key / built / tab / need -- for env b (b = -1: every env),
// or the batch's max_branch / Ucap / Rcap (an int per env asked for).  Returns the bytes of it (copied when they fit `cap`), -1: no such name or env.
extern "C" long long fl_debug_static_read(FlStatic *s, const char *name, int b, void *out, long long cap) {
    if (!s || !name || !out || b < -1 || b >= s->B) return -1;
    long long n = -1;
    auto array = [&](const char *is, const auto &v) {   // B equal slices
        if (strcmp(is, name) != 0) return;
        const size_t per_env = v.size() / s->B, first = b < 0 ? 0 : b * per_env, count = b < 0 ? v.size() : per_env;
        n = (long long)(count * sizeof v[0]);
        if (n <= cap) memcpy(out, v.data() + first, (size_t)n);
    };
    fl_static_host_arrays(*s, [&](const char *is, auto &host, size_t, int, bool) { array(is, host); });
    array("grid", s->grid); array("ut", s->ut); array("maxbr", s->maxbr); array("loaded", s->loaded); array("dirty", s->dirty);
    array("key", s->key); array("built", s->built); array("tab", s->tab); array("need", s->need);
    array("max_branch", std::vector<int>(s->B, fl_static_max_branch(*s)));
    array("Ucap", std::vector<int>(s->B, s->Ucap)); array("Rcap", std::vector<int>(s->B, s->Rcap));
    return n;
}

// diagnostic, no HIP call: a window on the constexpr tables of fl_policy_layout.h.  table 0 = saved_dev's arrays, 1 = rows_dev's: name,
// *a = floats a row, *b = floats a row before it; table 2 = the head's parameters: *a = out, *b = in (0: a bias), name "bf16" for a matrix
// fl_policy_head_pack_bf16 rounds, else "".  i < 0: returns the table's entries; else fills entry i and returns 0; -1: no such table or entry.
extern "C" int fl_debug_policy_layout(int table, int i, char *name, int name_cap, int *a, int *b) {
    const int count = table == 0 ? FPL_S_COUNT : table == 1 ? FPL_R_COUNT : table == 2 ? FPH_NPARAMS : -1;
    if (i < 0 || count < 0) return count;
    if (i >= count || !name || name_cap < 1 || !a || !b) return -1;
    const FplArray *t = table == 0 ? FPL_SAVED : FPL_ROWS;
    if (table == 2) { *a = FPL_PARAMS[i].out; *b = FPL_PARAMS[i].in; }
    else { *a = t[i].floats; *b = fpl_before(t, i); }
    snprintf(name, (size_t)name_cap, "%s", table == 2 ? (FPL_PARAMS[i].bf16 ? "bf16" : "") : t[i].name);
    return 0;
}

double fl_algorithmic_bytes_per_agent_step(fl_batch *h, int with_cutils_obs, int tree_depth) {
    if (!h) return 0.0;
    // DESIGN.md "algorithmic bytes": compulsory HBM traffic per agent-step with this SoA.
    //   dynamics: 20 B state read + 20 B state write + 16 B static read (init_pos, target, earliest, spk; latest/speed/tslot
    //             only on the terminal step) + 1 B action + 5 B reward/done + 8 B RNG words + MT block write amortised
    //             (2496 B / 312 agent-steps = 8 B)
    //   per env amortised over A: rail grid 2*H*W read once per obs build
    //   cutils obs out: 31*12*4 + 30*3*4 + 31*4 + 30*4 + 83*4 + 5 = 2429 B; depth-d tree out: 12*8*N(d) (f64)
    double bytes = 20 + 20 + 16 + 1 + 5 + 8 + 8;
    if (with_cutils_obs || tree_depth > 0) bytes += 2.0 * h->s.H * h->s.W / h->s.A;
    if (with_cutils_obs) bytes += 2429.0 + 20 + 36 + 2 * 31;  // + state/static re-read by the obs kernel + 31 distance-map gathers
    if (tree_depth > 0) {
        int n = 1, p = 1;
        for (int k = 0; k < tree_depth; k++) { p *= 4; n += p; }
        bytes += 96.0 * n + 2.0 * n;
    }
    return bytes;
}
