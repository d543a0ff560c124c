"""EXTENSION (not reference behaviour): tracklets of an unlabeled capture whose marker columns change identity.

The reference -- and every layer built on it -- assumes that a marker column holds ONE physical marker for the whole capture.
A raw unlabeled capture is a set of tracklets: a slot loses its marker and is reused for another one, and two trajectories may
exchange slots when they pass each other.  `segment_tracklets` cuts every column into tracklets with three rules on the visible
entries (get_marker_mask's rule: an entry of exact zeros is missing), walked in frame order.  A new tracklet begins

  * at the column's first visible entry,
  * after more than `max_gap` consecutive missing frames,
  * where |x_f - x_prev| > max_jump (f - f_prev), `prev` being the previous visible entry of the column,

and tracklets with fewer than `min_length` visible entries are dropped.  Host logic on whatever device the markers live on:
scans (cummax / cumsum), a gather and a bincount -- no Python loop over the frames.

Config key (off when absent):  stages.compute_locations.tracklets: {max_gap: frames, max_jump: metres per frame,
min_length: frames}.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch


@dataclass
class Tracklets:
    """`seg` [F, M] int32: the tracklet id of every entry, -1 where there is none.  Ids are dense, 0..S-1, ordered by
    (column, start).  `column`, `start`, `stop` [S] int64: the tracklet's column, its first visible frame and one past its
    last visible frame."""

    seg: torch.Tensor
    column: torch.Tensor
    start: torch.Tensor
    stop: torch.Tensor

    @property
    def count(self) -> int:
        return int(self.column.numel())

    def columns_with_events(self) -> torch.Tensor:
        """[M] bool: columns that hold more than one tracklet."""
        M = self.seg.shape[1]
        return torch.bincount(self.column, minlength=M) > 1


def _from_starts(vis: torch.Tensor, starts: torch.Tensor, min_length: int) -> Tracklets:
    """Tracklets of the visible entries `vis` [F, M] that begin at `starts` [F, M] (a subset of vis with every column's first
    visible entry in it): dense ids by (column, start), tracklets under `min_length` visible entries dropped."""
    F, M = vis.shape
    dev = vis.device
    per_col = starts.sum(dim=0)                                             # [M] tracklets per column
    col_off = torch.cumsum(per_col, dim=0) - per_col                        # exclusive scan: first id of the column
    raw = torch.cumsum(starts.long(), dim=0) - 1 + col_off[None, :]         # [F, M] id of the run the entry is in
    n_raw = int(per_col.sum())
    raw_v = raw[vis]
    length = torch.bincount(raw_v, minlength=n_raw)                         # visible entries per tracklet
    keep = length >= int(min_length)
    new_id = torch.cumsum(keep.long(), dim=0) - 1                           # dense again, order kept
    seg = torch.full((F, M), -1, dtype=torch.int32, device=dev)
    kept_entry = vis.clone()
    kept_entry[vis] = keep[raw_v]
    seg[kept_entry] = new_id[raw[kept_entry]].to(torch.int32)
    frame = torch.arange(F, device=dev)[:, None].expand(F, M)
    S = int(keep.sum())
    sid = seg[kept_entry].long()
    fr = frame[kept_entry]
    column = torch.zeros(S, dtype=torch.long, device=dev)
    start = torch.full((S,), F, dtype=torch.long, device=dev)
    stop = torch.zeros(S, dtype=torch.long, device=dev)
    if S:
        col = torch.arange(M, device=dev)[None, :].expand(F, M)[kept_entry]
        column.scatter_(0, sid, col)
        start.scatter_reduce_(0, sid, fr, reduce="amin")
        stop.scatter_reduce_(0, sid, fr + 1, reduce="amax")
    return Tracklets(seg=seg, column=column, start=start, stop=stop)


def segment_tracklets(markers: torch.Tensor, max_gap: int, max_jump: float, min_length: int) -> Tracklets:
    """Tracklets of `markers` [F, M, 3] (see the module docstring for the rule)."""
    if markers.dim() != 3 or markers.shape[2] != 3:
        raise ValueError("segment_tracklets: markers [F, M, 3] expected")
    max_gap, max_jump, min_length = _check_params(max_gap, max_jump, min_length, "segment_tracklets")
    F, M = int(markers.shape[0]), int(markers.shape[1])
    dev = markers.device
    vis = torch.sum(torch.abs(markers), dim=-1) != 0.0                      # get_marker_mask's rule
    frame = torch.arange(F, device=dev)[:, None].expand(F, M)
    last_vis = torch.cummax(torch.where(vis, frame, torch.full_like(frame, -1)), dim=0)[0]   # last visible frame <= f
    prev = torch.cat([torch.full((1, M), -1, dtype=last_vis.dtype, device=dev), last_vis[:-1]], dim=0)  # ... < f
    has_prev = prev >= 0
    x = markers.double()
    x_prev = torch.gather(x, 0, prev.clamp(min=0)[..., None].expand(F, M, 3))
    dt = (frame - prev).double()
    jump = torch.linalg.norm(x - x_prev, dim=-1) > float(max_jump) * dt
    gap = (frame - prev - 1) > max_gap
    starts = vis & (~has_prev | gap | jump)
    return _from_starts(vis, starts, min_length)


def tracklets_from_identity(identity: torch.Tensor, min_length: int = 1) -> Tracklets:
    """Ground-truth tracklets of a table of physical-marker ids [F, M] (-1 = missing): a tracklet is a run of consecutive
    frames of one column that shows one marker without a missing frame in it.  Same id ordering and `min_length` rule as
    segment_tracklets."""
    identity = torch.as_tensor(identity).long()
    vis = identity >= 0
    before = torch.cat([torch.full_like(identity[:1], -1), identity[:-1]], dim=0)
    starts = vis & (identity != before)
    return _from_starts(vis, starts, min_length)


def _check_params(max_gap, max_jump, min_length, where: str):
    def as_int(v, name, lo):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or float(v) != int(v) or int(v) < lo:
            raise ValueError("%s.%s must be an integer >= %d (got %r)" % (where, name, lo, v))
        return int(v)

    g = as_int(max_gap, "max_gap", 0)
    n = as_int(min_length, "min_length", 1)
    if isinstance(max_jump, bool) or not isinstance(max_jump, (int, float)) or not math.isfinite(float(max_jump)) \
            or float(max_jump) <= 0.0:
        raise ValueError("%s.max_jump must be a positive finite number of metres per frame (got %r)" % (where, max_jump))
    return g, float(max_jump), n


def tracklets_config(config: Dict) -> Optional[Dict]:
    """stages.compute_locations.tracklets of a config, checked: None when the key is absent (the extension is off), else
    {"max_gap": int >= 0, "max_jump": float > 0, "min_length": int >= 1}.  ValueError with the key's path otherwise."""
    path = "stages.compute_locations.tracklets"
    t = (config["stages"].get("compute_locations") or {}).get("tracklets")
    if t is None:
        return None
    if not isinstance(t, dict) or set(t) != {"max_gap", "max_jump", "min_length"}:
        raise ValueError("%s must be a mapping with exactly the keys max_gap, max_jump, min_length (got %r)" % (path, t))
    g, j, n = _check_params(t["max_gap"], t["max_jump"], t["min_length"], path)
    return {"max_gap": g, "max_jump": j, "min_length": n}
