// fl_policy_host.h -- the checks and the launch tail that the entry points of fl_tree_lstm.hip and fl_policy_head.hip share.  Host
// code only; every check runs before the caller's first HIP call.  `fn` names the entry point in the message.
#pragma once
#include <stdio.h>

#include "fl_internal.h"
#include "fl_policy_layout.h"

// (n_envs, n_agents) of the head's entry points: a row index times an array's width stays inside an int
static inline int fph_check_sizes(const char *fn, int n_envs, int n_agents) {
    if (n_envs <= 0 || n_agents < 1 || n_agents > FPH_MAX_A || (long long)n_envs * n_agents > INT32_MAX / (3 * FPH_E)) {
        fl_set_error("%s: bad sizes (n_envs %d, n_agents %d; 1 <= n_envs, 1 <= n_agents <= %d)", fn, n_envs, n_agents, FPH_MAX_A);
        return FL_ERR_ARG;
    }
    return FL_OK;
}

struct FlPtr {
    const void *p;
    const char *name;
    int align;
    bool may_be_null;
};

// the pointers' NULLs and alignment, in the table's order
static inline int fl_check_ptrs(const char *fn, const FlPtr *tab, int n) {
    for (int i = 0; i < n; i++) {
        if (!tab[i].p && !tab[i].may_be_null) { fl_set_error("%s: %s is NULL", fn, tab[i].name); return FL_ERR_ARG; }
        if ((uintptr_t)tab[i].p % tab[i].align) {
            fl_set_error("%s: %s is not %d-byte aligned", fn, tab[i].name, tab[i].align);
            return FL_ERR_ARG;
        }
    }
    return FL_OK;
}

// parameter i of a list of float32 parameters: there, and 16-byte aligned
static inline int fl_check_param(const char *fn, const float *const *params, int i) {
    char name[32];
    snprintf(name, sizeof name, "parameter %d", i);
    const FlPtr t = {params[i], name, 16};
    return fl_check_ptrs(fn, &t, 1);
}

// a buffer (`what`: "workspace", "packed buffer", ...) of `have` bytes where `sizer` asks for `need`
static inline int fl_check_bytes(const char *fn, const char *what, size_t have, size_t need, const char *sizer) {
    if (have < need) {
        fl_set_error("%s: %s of %zu bytes, %zu needed (%s)", fn, what, have, need, sizer);
        return FL_ERR_ARG;
    }
    return FL_OK;
}

// behind the last launch of an entry point
static inline int fl_launched(const char *fn) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { fl_set_error("%s: launch failed: %s", fn, hipGetErrorString(e)); return FL_ERR_HIP; }
    return FL_OK;
}
