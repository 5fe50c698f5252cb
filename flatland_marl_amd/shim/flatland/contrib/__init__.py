"""flatland.contrib: the wrappers of flatland/contrib/wrappers/flatland_wrappers.py (see flatland_marl_amd/shim/__init__.py)"""
