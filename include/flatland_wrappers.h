/* flatland_wrappers.h -- the reduced action space of flatland/contrib/wrappers/flatland_wrappers.py as device outputs.
 * Exported by libflatland_hip.so next to include/flatland_hip.h (whose handle, error codes, FL_ACTION_ABSENT and fl_last_error this
 * uses; a header of its own, as flatland_policy.h, flatland_train.h and flatland_predict.h are, so that flatland_hip.h stays the
 * list it was).
 *
 * fl_action_space: for every agent of the envs [b0, b0 + nb), one launch on the handle's stream, no host synchronisation, no
 * allocation.  Device outputs:
 *   sp_action_dev   u8 [nb][A][3]  the RailEnvActions of possible_actions_sorted_by_distance(env, handle)
 *                                  (flatland_wrappers.py:14-56): the transitions of (virtual position, direction) in N, E, S, W
 *                                  order (:32-48; MOVE_FORWARD also for the turn in a dead end, :40-45), stably sorted by distance
 *                                  (:49), a single candidate doubled (:53-54), (DO_NOTHING, 0) twice for WAITING,
 *                                  MALFUNCTION_OFF_MAP and DONE (:21-26); 0 behind the list
 *   sp_dist_dev     [nb][A][3]     their distances, distance_map.get()[handle][new position + (movement,)] (:30, :47);
 *                                  elem_kind 0 = float64 with inf (the reference's values), 1 = int32 with INT32_MAX for inf;
 *                                  infinity behind the list, and for a neighbour off the grid or without rail
 *   sp_count_dev    u8 [nb][A]     the list's length: 2 or 3 on valid maps
 *   on_decision_dev u8 [nb][A]     SkipNoChoiceCellsWrapper.on_decision_cell(agent) (:197-198): position None, position ==
 *                                  initial_position, or position in decision_cells
 *   actions_dev     u8 [nb][A]     ShortestPathActionWrapper.step's translation (:131-138) of reduced_dev u8 [nb][A]: 0 -> 0,
 *                                  a >= 1 -> the action of entry a - 1, FL_ACTION_ABSENT (an agent not in the dict) -> itself;
 *                                  what fl_step takes.  a - 1 >= count gives 0 where the reference raises IndexError.
 * sp_action_dev, sp_dist_dev and sp_count_dev are given together or not at all, reduced_dev and actions_dev likewise;
 * on_decision_dev may be NULL.  Every element of every given output is written.
 * FL_ERR_ARG before any HIP call: a bad range, elem_kind outside 0 .. 1, every output NULL, sp_action_dev / sp_dist_dev /
 * sp_count_dev not given together, reduced_dev without actions_dev or the reverse, a float64 sp_dist_dev that is not 8-byte
 * aligned (int32: 4-byte), an uncommitted handle.
 *
 * fl_decision_cells: find_all_cells_where_agent_can_choose(env) (flatland_wrappers.py:145-176) of the envs [b0, b0 + nb) as
 * cells_dev u8 [nb][H][W]: bit 0 = the cell is in `switches` (:158-166), bit 1 = in `switches_neighbors` (:167-173), non-zero = in
 * `decision_cells` (:175).  The table is built with the env's static tables (commit, replace_env); the call is one launch (a
 * gather through the owners of shared tables) on the handle's stream, no host synchronisation, no allocation.  Cells without rail are 0.  FL_ERR_ARG before any HIP call: a bad range, cells_dev NULL, an uncommitted handle. */
#ifndef FLATLAND_WRAPPERS_H
#define FLATLAND_WRAPPERS_H
#include "flatland_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fl_action_space(fl_batch *h, int b0, int nb, int elem_kind, uint8_t *sp_action_dev, void *sp_dist_dev, uint8_t *sp_count_dev,
                    uint8_t *on_decision_dev, const uint8_t *reduced_dev, uint8_t *actions_dev);
int fl_decision_cells(fl_batch *h, int b0, int nb, uint8_t *cells_dev);

#ifdef __cplusplus
}
#endif
#endif
