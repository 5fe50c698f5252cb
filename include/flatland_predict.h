/* flatland_predict.h -- the shortest-path predictor as an output of its own.
 * Exported by libflatland_hip.so next to include/flatland_hip.h (whose handle, error codes and fl_last_error this uses; a header of
 * its own, as flatland_policy.h and flatland_train.h are, so that flatland_hip.h stays the list it was).
 *
 * fl_predict: flatland.envs.predictions.ShortestPathPredictorForRailEnv(max_depth).get() and get_shortest_paths(distance_map, max_depth) for every
 * agent of the envs [b0, b0 + nb) (flatland/envs/predictions.py:97-180, rail_env_shortest_paths.py:203-274), one launch on the
 * handle's stream, no host synchronisation, no allocation.  Device outputs:
 *   pred_dev     [nb][A][max_depth + 1][5]  rows (time, row, col, direction, action); elem_kind 0 = float64 (the reference's dtype),
 *                                           1 = int32 (the same values)
 *   path_dev     i32 [nb][A][max_depth][3]  (row, col, direction) of the waypoints get_shortest_paths returns, -1 behind the path
 *   path_len_dev i32 [nb][A]                their number; 0 = the reference's None
 * pred_dev may be NULL, or path_dev and path_len_dev together, not all three.  Every element of every given output is written.
 * FL_ERR_ARG before any HIP call: a bad range, max_depth outside 1 .. 500, elem_kind outside 0 .. 1, every output NULL, path_dev
 * without path_len_dev or the reverse, pred_dev not 16-byte aligned.  cfg5 (256 envs of 400 agents) at depth 500 is 2 GB in float64:
 * take big batches in env ranges. */
#ifndef FLATLAND_PREDICT_H
#define FLATLAND_PREDICT_H
#include "flatland_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fl_predict(fl_batch *h, int b0, int nb, int max_depth, int elem_kind, void *pred_dev, int32_t *path_dev, int32_t *path_len_dev);

#ifdef __cplusplus
}
#endif
#endif
