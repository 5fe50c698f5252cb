"""flatland.contrib.wrappers (an empty package in the reference too)"""
