"""Experiment drivers (mirrors pldepth/run_scripts)."""
