"""YAML configuration with single-parent inheritance (reference utils/config.py:6-18).

``parent:`` is a path; the reference resolves it relative to the CWD (``config/video_mocap.yaml``).  Here it is
tried relative to the CWD first and then relative to the directory that holds the packaged configs, so both
the reference's files and the packaged copies load.  Child keys deep-merge over the parent's (mergedeep
semantics for nested dicts: dicts merge recursively, everything else is replaced).
"""
from __future__ import annotations

import copy
import math
import os
from typing import Dict

import yaml

CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config")


def deep_merge(dst: Dict, *srcs: Dict) -> Dict:
    for src in srcs:
        for key, val in src.items():
            if isinstance(val, dict) and isinstance(dst.get(key), dict):
                deep_merge(dst[key], val)
            else:
                dst[key] = copy.deepcopy(val)
    return dst


def _resolve(path: str) -> str:
    if os.path.isfile(path):
        return path
    alt = os.path.join(os.path.dirname(CONFIG_DIR), path)
    if os.path.isfile(alt):
        return alt
    alt = os.path.join(CONFIG_DIR, os.path.basename(path))
    if os.path.isfile(alt):
        return alt
    raise FileNotFoundError(path)


def load_config(filename: str) -> Dict:
    with open(_resolve(filename), "r") as stream:
        try:
            output = yaml.safe_load(stream)
        except yaml.YAMLError as error:  # the reference prints and returns None (utils/config.py:16-18)
            print(error)
            return None
    if output.get("parent") is not None:
        output = deep_merge({}, load_config(output["parent"]), output)
    return output


def packaged_config(name: str = "video_mocap") -> Dict:
    """One of the packaged flag sets: video_mocap | hmr_full | hmr_part | mht_rotation."""
    return load_config(os.path.join(CONFIG_DIR, name + ".yaml"))


def stage_surface(config: Dict):
    """EXTENSION: the point-to-surface data term of the chamfer stage (uuo_problem_t.surface) as (weight, stand-off in metres):
    stages.chamfer.losses.surface_chamfer and stages.chamfer.surface_distance (absent = 0).  Weight 0 or absent = off.  The term
    REPLACES the vertex term `full_chamfer`: a config that names both with a non-zero weight is refused, and so are the
    soft-assignment term `soft_chamfer` beside it, negative or non-finite weights and negative or non-finite stand-offs."""
    st = config["stages"]["chamfer"]
    losses = st.get("losses") or {}
    from .terms import _weight  # (the extension terms' one weight check)

    w = _weight(config, "chamfer", "surface_chamfer")
    d0 = st.get("surface_distance", 0.0)
    d0 = 0.0 if d0 is None else float(d0)
    if not math.isfinite(d0) or d0 < 0.0:
        raise ValueError("stages.chamfer.surface_distance must be a finite number of metres >= 0 (got %r)" % (d0,))
    if w > 0.0 and float(losses.get("full_chamfer", 0.0) or 0.0) != 0.0:
        raise ValueError("stages.chamfer.losses: surface_chamfer replaces full_chamfer (the point-to-surface term is the stage's "
                         "data term); name one of them, not both")
    if w > 0.0 and float(losses.get("soft_chamfer", 0.0) or 0.0) != 0.0:
        raise NotImplementedError("stages.chamfer: surface_chamfer (point-to-surface term) is not built for the soft-assignment "
                                  "term soft_chamfer; use one or the other")
    return w, d0
