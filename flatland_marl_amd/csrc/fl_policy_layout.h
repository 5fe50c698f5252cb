// fl_policy_layout.h -- the code's one copy of what the policy network's host code has to agree on: the sizes, the shapes of the
// head's 38 and the encoder's 8 parameters, and the order and width of the arrays of saved_dev and rows_dev
// (include/flatland_policy_train.h has the same in prose).  Constants, constexpr tables and constexpr functions only: no kernel, no
// device code, no HIP call.  Included by fl_policy_head.h, fl_tree_lstm.h and fl_policy_host.h, so by every unit of the policy.
// hip_backend.py states the same tables for Python; tests/test_policy_layout.py holds the two equal through fl_debug_policy_layout.
#pragma once
#include <stddef.h>

#include "../../include/flatland_policy_train.h"

#define FPH_ATTR 83
#define FPH_H 128                   // hidden_sz = tree_embedding_sz
#define FPH_E 256                   // embedding
#define FPH_ACT 5
#define FPH_NPARAMS 38
#define FPH_MAX_A 1024
#define FTL_F 12                    // the encoder: features a node
#define FTL_M 128                   // ... and its hidden size
#define FTL_NPARAMS 8

// ---------------------------------------------------------------------------------------------------------------- parameters
// a parameter in state_dict order: a weight [out][in], or a bias [out] (in = 0); bf16: one of the matrices fl_policy_head_pack_bf16 rounds
struct FplParam { int out, in; bool bf16; };
#define FPL_LAYER(out, in, bf16) {out, in, bf16}, {out, 0, false}
#define FPL_BLOCK FPL_LAYER(3 * FPH_E, FPH_E, true), FPL_LAYER(FPH_E, FPH_E, true), FPL_LAYER(FPH_E, 2 * FPH_E, true)     // in_proj, out_proj, att_mlp.0
#define FPL_HEAD(last) FPL_LAYER(FPH_E, 2 * FPH_E, true), FPL_LAYER(FPH_H, FPH_E, true), FPL_LAYER(last, FPH_H, false)
static constexpr FplParam FPL_PARAMS[FPH_NPARAMS] = {
    FPL_LAYER(FPH_E, FPH_ATTR, false), FPL_LAYER(FPH_E, FPH_E, true), FPL_LAYER(FPH_E, FPH_E, true), FPL_LAYER(FPH_H, FPH_E, true),   // attr_embedding
    FPL_BLOCK, FPL_BLOCK, FPL_BLOCK,                                                                                                  // transformer.0 .. 2
    FPL_HEAD(FPH_ACT), FPL_HEAD(1),                                                                                                   // actor_net, critic_net
};
// the encoder's: W_iou, b_iou, U_iou, W_c, b_c, W_f, b_f, U_f
static constexpr FplParam FTL_PARAMS[FTL_NPARAMS] = {
    FPL_LAYER(3 * FTL_M, FTL_F, false), {3 * FTL_M, 3 * FTL_M, false}, FPL_LAYER(FTL_M, 3 * FTL_M, false), FPL_LAYER(FTL_M, FTL_F, false),
    {FTL_M, FTL_M, false},
};
#undef FPL_HEAD
#undef FPL_BLOCK
#undef FPL_LAYER

// the float64 partial sums a slice of the parameter-gradient kernel keeps for these parameters: one for every element
constexpr long long fpl_elements(const FplParam *t, int n) {
    long long s = 0;
    for (int i = 0; i < n; i++) s += (long long)t[i].out * (t[i].in ? t[i].in : 1);
    return s;
}
constexpr long long FPG_HEAD_DOUBLES = fpl_elements(FPL_PARAMS, FPH_NPARAMS), FPG_TREE_DOUBLES = fpl_elements(FTL_PARAMS, FTL_NPARAMS);
static_assert(FPG_HEAD_DOUBLES == 1698694 && FPG_TREE_DOUBLES == 219776, "fl_*_param_grads_workspace_bytes a slice, as documented");

// the parameter index of the m-th packed bf16 matrix (-1: there are fewer), and the packed buffer's elements before it
constexpr int fpl_bf16_param(int m) {
    for (int i = 0; i < FPH_NPARAMS; i++)
        if (FPL_PARAMS[i].bf16 && m-- == 0) return i;
    return -1;
}
constexpr int fpl_bf16_before(int m) {
    int s = 0;
    for (int k = 0; k < m; k++) s += FPL_PARAMS[fpl_bf16_param(k)].out * FPL_PARAMS[fpl_bf16_param(k)].in;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- saved_dev, rows_dev
// X(enumerator, name, floats a row), in the buffer's order; the names are hip_backend.POLICY_SAVED_LAYOUT's and POLICY_ROWS_LAYOUT's
#define FPL_SAVED_ARRAYS(X)                                                                                                            \
    X(EMB, "emb", FPH_E) X(Y1, "y1", FPH_E) X(Y2, "y2", FPH_E) X(Y3, "y3", FPH_E)                                                      \
    X(C0, "c0", FPH_E) X(C1, "c1", FPH_E) X(C2, "c2", FPH_E)                                                                           \
    X(QKV0, "qkv0", 3 * FPH_E) X(QKV1, "qkv1", 3 * FPH_E) X(QKV2, "qkv2", 3 * FPH_E)                                                   \
    X(VAL, "val", 1)
#define FPL_ROWS_BLOCK(X, i)                                                                                                           \
    X(DQKV##i, "dqkv" #i, 3 * FPH_E) X(DO##i, "do" #i, FPH_E) X(DZ##i, "dz" #i, FPH_E) X(O##i, "o" #i, FPH_E) X(DC##i, "dc" #i, FPH_E) \
    X(DY##i, "dy" #i, FPH_E)
#define FPL_ROWS_HEAD(X, H, h, last)     /* last: the last layer's dZ, zero filled to a multiple of 4 floats */                        \
    X(H##_DZ0, h ".dz0", FPH_E) X(H##_DZ2, h ".dz2", FPH_H) X(H##_DZ4, h ".dz4", last) X(H##_U1, h ".u1", FPH_E) X(H##_U2, h ".u2", FPH_H)
#define FPL_ROWS_ARRAYS(X)                                                                                                             \
    X(ATTR_DZ0, "attr.dz0", FPH_E) X(ATTR_DZ2, "attr.dz2", FPH_E) X(ATTR_DZ4, "attr.dz4", FPH_E) X(ATTR_DZ6, "attr.dz6", FPH_H)        \
    X(ATTR_H1, "attr.h1", FPH_E) X(ATTR_H2, "attr.h2", FPH_E) X(ATTR_H3, "attr.h3", FPH_E)                                             \
    FPL_ROWS_BLOCK(X, 0) FPL_ROWS_BLOCK(X, 1) FPL_ROWS_BLOCK(X, 2)                                                                     \
    X(DY3, "dy3", FPH_E)                                                                                                               \
    FPL_ROWS_HEAD(X, ACTOR, "actor", 8) FPL_ROWS_HEAD(X, CRITIC, "critic", 4)

struct FplArray { const char *name; int floats; };
#define FPL_ENUM_S(id, name, floats) FPL_S_##id,
#define FPL_ENUM_R(id, name, floats) FPL_R_##id,
#define FPL_ENTRY(id, name, floats) {name, floats},
enum FplSaved { FPL_SAVED_ARRAYS(FPL_ENUM_S) FPL_S_COUNT };
enum FplRows { FPL_ROWS_ARRAYS(FPL_ENUM_R) FPL_R_COUNT };
static constexpr FplArray FPL_SAVED[FPL_S_COUNT] = {FPL_SAVED_ARRAYS(FPL_ENTRY)};
static constexpr FplArray FPL_ROWS[FPL_R_COUNT] = {FPL_ROWS_ARRAYS(FPL_ENTRY)};
#undef FPL_ENTRY
#undef FPL_ENUM_R
#undef FPL_ENUM_S
enum {                                                       // (saved: FPL_S_EMB + i = y_i, FPL_S_C0 + i, FPL_S_QKV0 + i are block i's)
    FPL_R_PER_BLOCK = FPL_R_DQKV1 - FPL_R_DQKV0,             // FPL_R_DQKV0 + i * FPL_R_PER_BLOCK: block i's
    FPL_R_PER_HEAD = FPL_R_CRITIC_DZ0 - FPL_R_ACTOR_DZ0,     // FPL_R_ACTOR_DZ0 + hd * FPL_R_PER_HEAD: the critic's for hd = 1
};
static_assert(FPL_S_COUNT == 11 && FPL_R_COUNT == 36, "11 saved arrays, 36 arrays of rows");

// the floats a row before array k: array k of a buffer of R rows starts at float R * before(k); before(count) = the floats a row
constexpr int fpl_before(const FplArray *t, int k) {
    int s = 0;
    for (int i = 0; i < k; i++) s += t[i].floats;
    return s;
}
constexpr int fpl_saved_before(int k) { return fpl_before(FPL_SAVED, k); }
constexpr int fpl_rows_before(int k) { return fpl_before(FPL_ROWS, k); }
constexpr int FPB_SAVED_FLOATS = fpl_saved_before(FPL_S_COUNT), FPB_ROW_FLOATS = fpl_rows_before(FPL_R_COUNT);
static_assert(FPB_SAVED_FLOATS == FL_POLICY_HEAD_SAVED_FLOATS && FPB_SAVED_FLOATS == 4097, "a row of saved_dev, as documented");
static_assert(FPB_ROW_FLOATS == FL_POLICY_HEAD_ROW_FLOATS && FPB_ROW_FLOATS == 9612, "a row of rows_dev, as documented");

// array k of a saved / rows buffer of R rows
template <class T>
static inline T *fpl_saved(T *buf, size_t R, int k) { return buf + R * fpl_saved_before(k); }
template <class T>
static inline T *fpl_rows(T *buf, size_t R, int k) { return buf + R * fpl_rows_before(k); }
