"""flatland.envs.observations: Node, the upstream TreeObsForRailEnv(max_depth, predictor) (observations.py:20-532) and
GlobalObsForRailEnv() (:535-611);
works on this library's RailEnv and, through the state hand-over of flatland_marl_amd.plugin, on any other env object"""
from flatland_marl_amd.rail_env import Node  # noqa: F401
from flatland_marl_amd.plugin import TreeObsUpstream
from flatland_marl_amd.plugin import GlobalObsForRailEnv as _GlobalObs


class TreeObsForRailEnv(TreeObsUpstream):
    def __init__(self, max_depth, predictor=None):
        super().__init__(max_depth, predictor)


class GlobalObsForRailEnv(_GlobalObs):
    def __init__(self):
        super().__init__()
