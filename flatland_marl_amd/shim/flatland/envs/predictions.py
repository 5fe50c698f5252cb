"""flatland.envs.predictions.ShortestPathPredictorForRailEnv(max_depth) (predictions.py:86-180): get() and get_shortest_paths() are
computed on the GPU (fl_predict); the tree builders still read only `max_depth` from it -- their prediction is part of the observation
kernel"""
from flatland_marl_amd.plugin import ShortestPathPredictorForRailEnv as _Predictor


class ShortestPathPredictorForRailEnv(_Predictor):
    def __init__(self, max_depth=20):
        super().__init__(max_depth)
