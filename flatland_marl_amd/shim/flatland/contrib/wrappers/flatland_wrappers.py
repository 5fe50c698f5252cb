"""flatland.contrib.wrappers.flatland_wrappers (flatland_wrappers.py:14-258): the shortest-path action space and the decision cells,
computed on the GPU (fl_action_space, fl_decision_cells) behind the reference's functions and wrapper classes"""
from flatland_marl_amd.rail_env import (  # noqa: F401
    RailEnvWrapper,
    ShortestPathActionWrapper,
    SkipNoChoiceCellsWrapper,
    find_all_cells_where_agent_can_choose,
    possible_actions_sorted_by_distance,
)

# DeadlockWrapper (flatland_wrappers.py:263-305) is absent on purpose.  Its Deadlock_Checker (contrib/utils/deadlock_checker.py)
# cannot be pinned to the reference: it asserts new_position == get_new_position(position, new_direction), which is false for every
# on-map agent whose action is DO_NOTHING or STOP_MOVING, so the reference raises there; and it reads env.agent_positions, which the
# reference updates incrementally (rail_env.py:360-367) and which therefore depends on the episode's history, not on the state.
# The library's own deadlock flags are the solution's: p_deadlocked of TreeObsForRailEnv.get_properties().
