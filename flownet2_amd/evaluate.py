"""Flow evaluation: the per-sample rows of the metrics kernel (csrc/flow_metrics.hip, include/flownet2_hip_flow_metrics.h), the numbers
a FlowNet user quotes computed from them, ground-truth readers, and the data-set loop of scripts/eval_flownet.py.

FlowMetrics holds one float64 row per sample in data-set order.  summary() is a pure function of those ordered rows, and a sample's row
does not depend on the batch it was computed in (the kernel's summation order follows (H, W) alone), so an evaluation gives the same
numbers, to the bit, for any batch size and any number of processes.

The KITTI flow PNG reader is written from the format's published description (the devkit's readme: 16-bit RGB, u = (R - 2^15) / 64,
v = (G - 2^15) / 64, valid = B != 0) and the PNG specification; no KITTI file was at hand to read with it.
"""
from __future__ import annotations

import math
import queue
import struct
import threading
import zlib

import numpy as np

from . import _lib, flo

_PREFIX = "FN2_FLOW_METRICS_"
_ENUM = _lib.FLOW_METRICS_CONSTANTS                                        # the header's enum, as the binding's parser read it
K = _ENUM[_PREFIX + "K"]
COLUMNS = tuple(sorted((n[len(_PREFIX):] for n in _ENUM if n != _PREFIX + "K"), key=lambda n: _ENUM[_PREFIX + n]))      # names in column order
COL = {name: i for i, name in enumerate(COLUMNS)}


def _ratio(num, den):
    return float(num) / float(den) if den != 0 else math.nan


class FlowMetrics:
    """The [n, K] float64 rows (columns COLUMNS) of n samples in data-set order; epe_map: the [n,1,H,W] map of the call that made them,
    where it was asked for."""

    def __init__(self, rows=None, epe_map=None):
        rows = np.zeros((0, K), np.float64) if rows is None else np.array(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != K:
            raise ValueError(f"FlowMetrics: rows must be [n, {K}], got {rows.shape}")
        self.rows = rows
        self.epe_map = epe_map

    def __len__(self):
        return self.rows.shape[0]

    def column(self, name):
        return self.rows[:, COL[name]]

    def merge(self, others):
        """This object's samples followed by those of `others`, in the order given."""
        return FlowMetrics(np.concatenate([self.rows] + [o.rows for o in others], axis=0))

    def summary(self):
        """The quoted numbers, in float64 from the rows:
          epe            mean over samples of each sample's mean EPE (Chairs, Sintel); samples without a counted pixel are left out
          epe_pixel      sum of EPE over the counted pixels of all samples / their number (KITTI; L1Loss's normalize_by_num_entries)
          fl_all         percent of counted pixels with EPE > outlier_abs and > outlier_rel |gt|
          ae_deg         mean angular error in degrees
          s0_10, s10_40, s40plus   mean EPE of the counted pixels in each band of |gt|
          epe_matched, epe_unmatched   mean EPE of the counted pixels outside / inside the occlusion mask
          epe_max, pixels (counted), samples, nonfinite (valid pixels with a NaN or Inf prediction: in no sum),
          samples_without_ground_truth (no valid pixel at all)
        A quotient with a zero denominator is nan (null in to_json's text)."""
        c = lambda name: self.column(name)
        tot = lambda name: float(np.sum(c(name)))
        valid = c("VALID")
        counted = valid > 0
        per_sample = c("EPE_SUM")[counted] / valid[counted]
        pixels, occ = tot("VALID"), tot("OCC_COUNT")
        return {
            "epe": _ratio(np.sum(per_sample), per_sample.size),
            "epe_pixel": _ratio(tot("EPE_SUM"), pixels),
            "fl_all": 100.0 * _ratio(tot("OUTLIERS"), pixels),
            "ae_deg": math.degrees(_ratio(tot("AE_SUM"), pixels)),
            "s0_10": _ratio(tot("BAND_EPE_SUM0"), tot("BAND_COUNT0")),
            "s10_40": _ratio(tot("BAND_EPE_SUM1"), tot("BAND_COUNT1")),
            "s40plus": _ratio(tot("BAND_EPE_SUM2"), tot("BAND_COUNT2")),
            "epe_matched": _ratio(tot("EPE_SUM") - tot("OCC_EPE_SUM"), pixels - occ),
            "epe_unmatched": _ratio(tot("OCC_EPE_SUM"), occ),
            "epe_max": float(np.max(c("EPE_MAX"))) if len(self) else math.nan,
            "pixels": int(pixels),
            "samples": len(self),
            "nonfinite": int(tot("NONFINITE")),
            "samples_without_ground_truth": int(np.sum((valid + c("NONFINITE")) == 0)),
        }

    def to_json(self, extra=None):
        """The summary and the per-sample rows as strict JSON; floats are written by repr, so the text is a function of the bits.
        extra: further top-level entries, written after the three."""
        import json
        return json.dumps({"summary": json_ready(self.summary()), "columns": list(COLUMNS), "rows": self.rows.tolist(), **(extra or {})}, indent=1,
                          allow_nan=False) + "\n"


def json_ready(summary):
    """A summary with null where a quotient had a zero denominator: JSON has no NaN, and a strict parser refuses the bare token."""
    return {k: None if isinstance(v, float) and math.isnan(v) else v for k, v in summary.items()}


def exit_status(summary, allow_nonfinite=False):
    """What scripts/eval_flownet.py exits with: 1 when a valid pixel had a NaN or Inf prediction (such pixels are in no sum, so the
    numbers look fine without them) unless that was allowed, else 0."""
    return 1 if summary["nonfinite"] > 0 and not allow_nonfinite else 0


# ---- forward-backward consistency -------------------------------------------------------------------------------------------------
_C_PREFIX = "FN2_FLOW_CONSISTENCY_"
_C_ENUM = _lib.FLOW_CONSISTENCY_CONSTANTS                                   # include/flownet2_hip_flow_consistency.h: columns and flag bits
CONSISTENCY_K = _C_ENUM[_C_PREFIX + "K"]
CONSISTENCY_FLAGS = {n[len(_C_PREFIX + "FLAG_"):]: v for n, v in _C_ENUM.items() if n.startswith(_C_PREFIX + "FLAG_")}      # name -> bit
CONSISTENCY_COLUMNS = tuple(sorted((n[len(_C_PREFIX):] for n in _C_ENUM if n != _C_PREFIX + "K" and not n.startswith(_C_PREFIX + "FLAG_")),
                                   key=lambda n: _C_ENUM[_C_PREFIX + n]))
CONSISTENCY_COL = {name: i for i, name in enumerate(CONSISTENCY_COLUMNS)}


class FlowConsistency:
    """The [n, K] float64 rows (columns CONSISTENCY_COLUMNS) of n samples per direction, in data-set order, and the maps of the call that
    made them: occ, flags, err, warped are (forward, backward) pairs or None.  Direction fw checks the forward flow against the backward
    one (occ_fw lives in frame 0, where the forward flow and its ground truth live), bw the reverse."""

    def __init__(self, rows_fw=None, rows_bw=None, occ=None, flags=None, err=None, warped=None, alpha=(0.01, 0.5), beta=(0.01, 0.002)):
        def rows(r, what):
            r = np.zeros((0, CONSISTENCY_K), np.float64) if r is None else np.array(r, dtype=np.float64)
            if r.ndim != 2 or r.shape[1] != CONSISTENCY_K:
                raise ValueError(f"FlowConsistency: {what} must be [n, {CONSISTENCY_K}], got {r.shape}")
            return r
        self.rows_fw, self.rows_bw = rows(rows_fw, "rows_fw"), rows(rows_bw, "rows_bw")
        if self.rows_fw.shape != self.rows_bw.shape:
            raise ValueError(f"FlowConsistency: {self.rows_fw.shape[0]} forward rows, {self.rows_bw.shape[0]} backward rows")
        pair = lambda p: (None, None) if p is None else tuple(p)
        (self.occ_fw, self.occ_bw), (self.flags_fw, self.flags_bw) = pair(occ), pair(flags)
        (self.err_fw, self.err_bw), (self.warped_fw, self.warped_bw) = pair(err), pair(warped)
        self.alpha, self.beta = (float(alpha[0]), float(alpha[1])), (float(beta[0]), float(beta[1]))

    def __len__(self):
        return self.rows_fw.shape[0]

    def merge(self, others):
        """This object's samples followed by those of `others`, in the order given (the rows; the maps stay with their calls)."""
        for o in others:
            if (o.alpha, o.beta) != (self.alpha, self.beta):
                raise ValueError(f"FlowConsistency.merge: thresholds differ ({o.alpha}, {o.beta} against {self.alpha}, {self.beta})")
        return FlowConsistency(np.concatenate([self.rows_fw] + [o.rows_fw for o in others], axis=0),
                               np.concatenate([self.rows_bw] + [o.rows_bw for o in others], axis=0), alpha=self.alpha, beta=self.beta)

    def sample(self, i):
        """Sample i alone (its rows)."""
        return FlowConsistency(self.rows_fw[i:i + 1], self.rows_bw[i:i + 1], alpha=self.alpha, beta=self.beta)

    @staticmethod
    def _direction(rows):
        tot = lambda name: float(np.sum(rows[:, CONSISTENCY_COL[name]]))
        pixels = tot("PIXELS")
        with_err = pixels - tot("OUTSIDE") - tot("NONFINITE")                   # the three flags that leave err NaN exclude one another
        return {
            "occluded": _ratio(tot("OCCLUDED"), pixels),
            "outside": _ratio(tot("OUTSIDE"), pixels),
            "inconsistent": _ratio(tot("INCONSISTENT"), pixels),
            "nonfinite": _ratio(tot("NONFINITE"), pixels),
            "boundary": _ratio(tot("BOUNDARY"), pixels),
            "err_mean": _ratio(tot("ERR_SUM"), with_err),
            "err_max": float(np.max(rows[:, CONSISTENCY_COL["ERR_MAX"]])) if rows.shape[0] else math.nan,
            "pixels": int(pixels),
        }

    def summary(self):
        """Per direction the fractions of all pixels that are occluded (outside, inconsistent or non-finite), outside, inconsistent,
        non-finite and on a motion boundary, the mean of err over the pixels that have one, the largest err and the pixel count; then
        the sample count and the thresholds.  A quotient with a zero denominator is nan (null in to_json's text)."""
        return {"fw": self._direction(self.rows_fw), "bw": self._direction(self.rows_bw), "samples": len(self), "alpha": list(self.alpha),
                "beta": list(self.beta)}

    def to_json(self):
        """The summary, one summary per sample (`lines`, in order) and the rows as strict JSON; floats are written by repr, so the text is
        a function of the bits."""
        import json
        ready = lambda s: {k: json_ready(v) if isinstance(v, dict) else v for k, v in s.items()}
        return json.dumps({"summary": ready(self.summary()), "lines": [ready(self.sample(i).summary()) for i in range(len(self))],
                           "columns": list(CONSISTENCY_COLUMNS), "rows_fw": self.rows_fw.tolist(), "rows_bw": self.rows_bw.tolist()}, indent=1,
                          allow_nan=False) + "\n"


# ---- unsupervised loss ---------------------------------------------------------------------------------------------------------------
_U_PREFIX = "FN2_UNSUP_LOSS_"
_U_ENUM = _lib.UNSUP_LOSS_CONSTANTS                                        # include/flownet2_hip_unsup_loss.h: the columns of a row
UNSUP_LOSS_K = _U_ENUM[_U_PREFIX + "K"]
UNSUP_LOSS_COLUMNS = tuple(sorted((n[len(_U_PREFIX):] for n in _U_ENUM if n != _U_PREFIX + "K"), key=lambda n: _U_ENUM[_U_PREFIX + n]))
UNSUP_LOSS_COL = {name: i for i, name in enumerate(UNSUP_LOSS_COLUMNS)}


class UnsupLoss:
    """The [n, K] float64 rows (columns UNSUP_LOSS_COLUMNS) of n samples per direction of functional.unsupervised_loss_report, and the
    loss of the call (None for rows put together by hand).  rows_bw is all zeros where no backward flow was given."""

    def __init__(self, rows_fw=None, rows_bw=None, loss=None, data_weight=1.0, smooth_weight=1.0, census=None):
        def rows(r, what):
            r = np.zeros((0, UNSUP_LOSS_K), np.float64) if r is None else np.array(r, dtype=np.float64)
            if r.ndim != 2 or r.shape[1] != UNSUP_LOSS_K:
                raise ValueError(f"UnsupLoss: {what} must be [n, {UNSUP_LOSS_K}], got {r.shape}")
            return r
        self.rows_fw = rows(rows_fw, "rows_fw")
        self.rows_bw = rows(rows_bw if rows_bw is not None else np.zeros_like(self.rows_fw), "rows_bw")
        if self.rows_fw.shape != self.rows_bw.shape:
            raise ValueError(f"UnsupLoss: {self.rows_fw.shape[0]} forward rows, {self.rows_bw.shape[0]} backward rows")
        self.loss = None if loss is None else float(loss)
        self.data_weight, self.smooth_weight = float(data_weight), float(smooth_weight)
        self.census = census                                                        # a CensusLoss where the census term is the data term

    def __len__(self):
        return self.rows_fw.shape[0]

    @staticmethod
    def _direction(rows):
        tot = lambda name: float(np.sum(rows[:, UNSUP_LOSS_COL[name]]))
        pixels = tot("PIXELS")
        return {
            "data_mean": _ratio(tot("DATA_SUM"), tot("COUNTED")),
            "smooth_mean": _ratio(tot("SMOOTH_SUM"), tot("SMOOTH_TERMS")),
            "counted": _ratio(tot("COUNTED"), pixels),
            "occluded": _ratio(tot("OCCLUDED"), pixels),
            "outside": _ratio(tot("OUTSIDE"), pixels),
            "nonfinite": _ratio(tot("NONFINITE"), pixels),
            "pixels": int(pixels),
        }

    def summary(self):
        """Per direction the mean data term over the counted pixels, the mean smoothness term, the shares of all pixels that were
        counted, occluded, outside and non-finite, and the pixel count; then the sample count, the weights and the loss.  A quotient with
        a zero denominator is nan.  Where the census term is the data term, its summary under "census"."""
        out = {"fw": self._direction(self.rows_fw), "bw": self._direction(self.rows_bw), "samples": len(self),
               "data_weight": self.data_weight, "smooth_weight": self.smooth_weight, "loss": self.loss}
        if self.census is not None:
            out["census"] = self.census.summary()
        return out


# ---- census data term ----------------------------------------------------------------------------------------------------------------
_C_PREFIX = "FN2_CENSUS_LOSS_"
_C_ENUM = _lib.CENSUS_LOSS_CONSTANTS                                      # include/flownet2_hip_census_loss.h: the columns of a row
CENSUS_LOSS_K = _C_ENUM[_C_PREFIX + "K"]
CENSUS_LOSS_COLUMNS = tuple(sorted((n[len(_C_PREFIX):] for n in _C_ENUM if n != _C_PREFIX + "K"), key=lambda n: _C_ENUM[_C_PREFIX + n]))
CENSUS_LOSS_COL = {name: i for i, name in enumerate(CENSUS_LOSS_COLUMNS)}


class CensusLoss:
    """The [n, K] float64 rows (columns CENSUS_LOSS_COLUMNS) of n samples per direction of functional.census_loss_report, and the loss of
    the call (None for rows put together by hand).  rows_bw is all zeros where no backward flow was given."""

    def __init__(self, rows_fw=None, rows_bw=None, loss=None, data_weight=1.0, radius=3):
        def rows(r, what):
            r = np.zeros((0, CENSUS_LOSS_K), np.float64) if r is None else np.array(r, dtype=np.float64)
            if r.ndim != 2 or r.shape[1] != CENSUS_LOSS_K:
                raise ValueError(f"CensusLoss: {what} must be [n, {CENSUS_LOSS_K}], got {r.shape}")
            return r
        self.rows_fw = rows(rows_fw, "rows_fw")
        self.rows_bw = rows(rows_bw if rows_bw is not None else np.zeros_like(self.rows_fw), "rows_bw")
        if self.rows_fw.shape != self.rows_bw.shape:
            raise ValueError(f"CensusLoss: {self.rows_fw.shape[0]} forward rows, {self.rows_bw.shape[0]} backward rows")
        self.loss = None if loss is None else float(loss)
        self.data_weight, self.radius = float(data_weight), int(radius)

    def __len__(self):
        return self.rows_fw.shape[0]

    @staticmethod
    def _direction(rows):
        tot = lambda name: float(np.sum(rows[:, CENSUS_LOSS_COL[name]]))
        pixels, counted = tot("PIXELS"), tot("COUNTED")
        return {
            "data_mean": _ratio(tot("DATA_SUM"), counted),
            "dist_mean": _ratio(tot("DIST_SUM"), counted),
            "pairs_mean": _ratio(tot("PAIRS"), counted),
            "counted": _ratio(counted, pixels),
            "occluded": _ratio(tot("OCCLUDED"), pixels),
            "outside": _ratio(tot("OUTSIDE"), pixels),
            "nonfinite": _ratio(tot("NONFINITE"), pixels),
            "pixels": int(pixels),
        }

    def summary(self):
        """Per direction the mean data term, the mean soft Hamming distance and the mean number of pairs over the counted pixels, the
        shares of all pixels that were counted, occluded, outside and non-finite, and the pixel count; then the sample count, the weight,
        the radius and the loss.  A quotient with a zero denominator is nan."""
        return {"fw": self._direction(self.rows_fw), "bw": self._direction(self.rows_bw), "samples": len(self),
                "data_weight": self.data_weight, "radius": self.radius, "loss": self.loss}


# ---- forward warping (splatting) -----------------------------------------------------------------------------------------------------
_S_PREFIX = "FN2_FLOW_SPLAT_"
_S_ENUM = _lib.FLOW_SPLAT_CONSTANTS                                        # include/flownet2_hip_flow_splat.h: columns, importances, statuses
FLOW_SPLAT_K = _S_ENUM[_S_PREFIX + "K"]
FLOW_SPLAT_STATUS = {n[len(_S_PREFIX + "STATUS_"):]: v for n, v in _S_ENUM.items() if n.startswith(_S_PREFIX + "STATUS_")}      # name -> byte
FLOW_SPLAT_COLUMNS = tuple(sorted((n[len(_S_PREFIX):] for n in _S_ENUM if n != _S_PREFIX + "K" and not n.startswith(_S_PREFIX + "STATUS_")
                                   and not n.startswith(_S_PREFIX + "IMPORTANCE_")), key=lambda n: _S_ENUM[_S_PREFIX + n]))
FLOW_SPLAT_COL = {name: i for i, name in enumerate(FLOW_SPLAT_COLUMNS)}


class FlowSplat:
    """The [n, K] float64 rows (columns FLOW_SPLAT_COLUMNS) of n samples of functional.flow_splat_report, and the planes of the call that
    made them (None for rows put together by hand): out, weight (the denominator), hole, status (uint8, FLOW_SPLAT_STATUS)."""

    def __init__(self, rows=None, out=None, weight=None, hole=None, status=None, t=1.0, mode="sum"):
        r = np.zeros((0, FLOW_SPLAT_K), np.float64) if rows is None else np.array(rows, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != FLOW_SPLAT_K:
            raise ValueError(f"FlowSplat: rows must be [n, {FLOW_SPLAT_K}], got {r.shape}")
        self.rows, self.out, self.weight, self.hole, self.status = r, out, weight, hole, status
        self.t, self.mode = float(t), str(mode)

    def __len__(self):
        return self.rows.shape[0]

    def summary(self):
        """The shares of all source pixels that were splatted, outside, masked and non-finite, the share of target cells that are holes,
        the mean of the weight plane over all cells and its maximum, the pixel and sample counts, the time and the mode.  A quotient with
        a zero denominator is nan."""
        tot = lambda name: float(np.sum(self.rows[:, FLOW_SPLAT_COL[name]]))
        pixels = tot("PIXELS")
        return {
            "splatted": _ratio(tot("SPLATTED"), pixels),
            "outside": _ratio(tot("OUTSIDE"), pixels),
            "masked": _ratio(tot("MASKED"), pixels),
            "nonfinite": _ratio(tot("NONFINITE"), pixels),
            "holes": _ratio(tot("HOLES"), pixels),
            "weight_mean": _ratio(tot("WEIGHT_SUM"), pixels),
            "weight_max": float(np.max(self.rows[:, FLOW_SPLAT_COL["WEIGHT_MAX"]])) if self.rows.shape[0] else math.nan,
            "pixels": int(pixels),
            "samples": len(self),
            "t": self.t,
            "mode": self.mode,
        }


def write_pgm(path, plane):
    """A [H,W] (or [1,H,W]) plane -> 8-bit binary PGM (P5, maxval 255): 255 where the plane is non-zero, else 0."""
    a = np.asarray(plane)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 2:
        raise ValueError(f"write_pgm: expected a [H,W] plane, got {a.shape}")
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(np.where(a != 0, 255, 0).astype(np.uint8).tobytes())


def bidirectional_names(out):
    """What the runners write beside the forward flow `out` (x.flo): (x.bw.flo, x.occ.pgm, x.bw.occ.pgm); a name without the .flo
    suffix is extended as it stands."""
    stem = out[:-4] if out.endswith(".flo") else out
    return stem + ".bw.flo", stem + ".occ.pgm", stem + ".bw.occ.pgm"


# ---- point trajectories -------------------------------------------------------------------------------------------------------------
_T_PREFIX = "FN2_FLOW_TRACK_"
_T_ENUM = _lib.FLOW_TRACK_CONSTANTS                                         # include/flownet2_hip_flow_track.h: columns and stop reasons
TRACK_K = _T_ENUM[_T_PREFIX + "K"]
TRACK_STOP = {n[len(_T_PREFIX + "STOP_"):]: v for n, v in _T_ENUM.items() if n.startswith(_T_PREFIX + "STOP_")}      # name -> state value
TRACK_COLUMNS = tuple(sorted((n[len(_T_PREFIX):] for n in _T_ENUM if n != _T_PREFIX + "K" and not n.startswith(_T_PREFIX + "STOP_")),
                             key=lambda n: _T_ENUM[_T_PREFIX + n]))
TRACK_COL = {name: i for i, name in enumerate(TRACK_COLUMNS)}
UNKNOWN_FLOW = 1e10                                                          # the .flo unknown-flow value (flow_metrics, flow_to_color skip it)


def _host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


class FlowTracks:
    """What one call of functional.flow_track (or several consecutive ones, merged) knows of P points per sample: rows [n, K] float64
    (columns TRACK_COLUMNS), tracks [n,F,2,P] (the position in every frame reached, NaN after; None where not asked for), start [n,2,P] the
    positions in the first frame, points [n,2,P] the last position reached, state uint8 [n,P] (0 = alive, else a TRACK_STOP value), steps
    int32 [n,P], size = (H, W) of the plane.  The arrays are torch tensors (on the device of the call) or NumPy arrays."""

    def __init__(self, rows=None, tracks=None, points=None, state=None, steps=None, start=None, size=None, alpha=(0.01, 0.5)):
        rows = np.zeros((0, TRACK_K), np.float64) if rows is None else np.array(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != TRACK_K:
            raise ValueError(f"FlowTracks: rows must be [n, {TRACK_K}], got {rows.shape}")
        self.rows, self.tracks, self.points, self.state, self.steps, self.start = rows, tracks, points, state, steps, start
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.alpha = (float(alpha[0]), float(alpha[1]))

    def __len__(self):
        return self.rows.shape[0]

    def column(self, name):
        return self.rows[:, TRACK_COL[name]]

    def merge(self, others):
        """This call followed by `others`, consecutive calls on the SAME points (each started from the points and state the one before
        returned): one object over all their frames.  tracks are joined along the frame axis (a later call's first frame is the earlier
        one's last), steps add, points and state are the last call's, start is the first one's.  Rows: POINTS the first call's, ALIVE the
        last one's, the stop reasons and STEPS_SUM add (exact integers), STEPS_MAX, DISP_SUM and DISP_MAX are computed anew from the
        merged steps, start and points -- the displacement in float32 as the kernel does, its sum in float64 in index order."""
        import torch
        calls = [self] + list(others)
        for o in calls:
            if o.alpha != self.alpha or o.size != self.size:
                raise ValueError(f"FlowTracks.merge: calls differ (alpha {o.alpha}, size {o.size} against {self.alpha}, {self.size})")
            if o.points is None or o.state is None or o.steps is None or o.start is None:
                raise ValueError("FlowTracks.merge: needs the points, state, steps and start of every call")
            if tuple(o.points.shape) != tuple(self.points.shape):
                raise ValueError(f"FlowTracks.merge: points {tuple(o.points.shape)} against {tuple(self.points.shape)}: not the same points")
        t = lambda a: torch.as_tensor(a)
        steps = t(calls[0].steps).clone()
        for o in calls[1:]:
            steps = steps + t(o.steps)
        tracks = None
        if all(o.tracks is not None for o in calls):
            tracks = torch.cat([t(calls[0].tracks)] + [t(o.tracks)[:, 1:] for o in calls[1:]], dim=1)
        last = calls[-1]
        rows = self.rows.copy()
        rows[:, TRACK_COL["ALIVE"]] = last.rows[:, TRACK_COL["ALIVE"]]
        for name in ("NONFINITE", "OUTSIDE", "INCONSISTENT", "MARKED", "STEPS_SUM"):
            rows[:, TRACK_COL[name]] = sum(o.rows[:, TRACK_COL[name]] for o in calls)
        s, p0, p1, alive = _host(steps), _host(self.start).astype(np.float32), _host(last.points).astype(np.float32), _host(last.state) == 0
        n = rows.shape[0]
        rows[:, TRACK_COL["STEPS_MAX"]] = s.reshape(n, -1).max(1) if s.size else 0
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1]
            d = np.where(alive, np.sqrt(dx * dx + dy * dy), np.float32(0)).astype(np.float64)
        rows[:, TRACK_COL["DISP_SUM"]] = [float(np.cumsum(r)[-1]) if r.size else 0.0 for r in d.reshape(n, -1)]
        rows[:, TRACK_COL["DISP_MAX"]] = d.reshape(n, -1).max(1) if d.size else 0
        return FlowTracks(rows, tracks=tracks, points=last.points, state=last.state, steps=steps, start=self.start, size=self.size, alpha=self.alpha)

    def summary(self):
        """Over all samples: the fraction of the points alive at the end and stopped by each reason, the mean and largest number of frames
        a point advanced, the mean (over the alive points) and largest displacement between the first and the last position, the point
        and sample counts.  A quotient with a zero denominator is nan."""
        tot = lambda name: float(np.sum(self.column(name)))
        points, alive = tot("POINTS"), tot("ALIVE")
        top = lambda name: float(np.max(self.column(name))) if len(self) else math.nan
        return {
            "alive": _ratio(alive, points),
            "nonfinite": _ratio(tot("NONFINITE"), points),
            "outside": _ratio(tot("OUTSIDE"), points),
            "inconsistent": _ratio(tot("INCONSISTENT"), points),
            "marked": _ratio(tot("MARKED"), points),
            "steps_mean": _ratio(tot("STEPS_SUM"), points),
            "steps_max": top("STEPS_MAX"),
            "disp_mean": _ratio(tot("DISP_SUM"), alive),
            "disp_max": top("DISP_MAX"),
            "points": int(points),
            "samples": len(self),
            "alpha": list(self.alpha),
        }

    def long_range_flow(self):
        """For a dense grid (P = H W, start = the pixel grid): the flow [n,2,H,W] from the first frame to the last, last position minus
        start, and 1e10 -- the .flo unknown-flow value, which flow_metrics and flow_to_color leave out -- where the point stopped."""
        if self.size is None or self.points is None or self.start is None or self.state is None:
            raise ValueError("FlowTracks.long_range_flow: needs size, start, points and state")
        H, W = self.size
        if tuple(self.points.shape[1:]) != (2, H * W):
            raise ValueError(f"FlowTracks.long_range_flow: points {tuple(self.points.shape)} are no dense grid on a {H} x {W} plane")
        if hasattr(self.points, "detach"):
            import torch
            d = torch.as_tensor(self.points) - torch.as_tensor(self.start).to(self.points.device)
            stopped = (torch.as_tensor(self.state).to(self.points.device) != 0).unsqueeze(1).expand_as(d)
            return torch.where(stopped, torch.full_like(d, UNKNOWN_FLOW), d).reshape(-1, 2, H, W)
        d = np.asarray(self.points, np.float32) - np.asarray(self.start, np.float32)
        stopped = np.broadcast_to((np.asarray(self.state) != 0)[:, None], d.shape)
        return np.where(stopped, np.float32(UNKNOWN_FLOW), d).astype(np.float32).reshape(-1, 2, H, W)


def track_names(out_dir):
    """What scripts/track_flownet.py writes into OUT_DIR: the trajectories (tracks.npz: pos float32 [F,2,P], NaN where a slot is empty;
    track_id int32 [F,P], -1 where empty; state uint8 [P])."""
    import os
    return os.path.join(out_dir, "tracks.npz")


def write_tracks_npz(path, pos, track_id, state):
    """tracks.npz with bytes that are a function of the arrays alone: the three of them in this order and with these types, stored
    uncompressed, every zip entry dated 1980-01-01 (np.savez would stamp them with the time of day).  np.load reads it."""
    import io
    import zipfile
    pos, track_id, state = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(track_id, np.int32), np.ascontiguousarray(state, np.uint8)
    if pos.ndim != 3 or pos.shape[1] != 2 or track_id.shape != (pos.shape[0], pos.shape[2]) or state.shape != (pos.shape[2],):
        raise ValueError(f"write_tracks_npz: pos {pos.shape} [F,2,P], track_id {track_id.shape} [F,P], state {state.shape} [P]")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in (("pos", pos), ("track_id", track_id), ("state", state)):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


# ---- the KITTI flow PNG -------------------------------------------------------------------------------------------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def _filter_row(ftype, row, prev, bpp):
    """PNG filter `ftype` of one scanline (bytes) given the unfiltered previous one (the writer is for fixtures: a Python step per byte)."""
    out = bytearray(len(row))
    for i, x in enumerate(row):
        a = row[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ftype]
        out[i] = (x - pred) & 255
    return out


def _unfilter(filtered, h, w, bpp):
    """The scanlines of a non-interlaced image (h rows of 1 filter-type byte + w * bpp bytes) -> uint8 [h, w, bpp], all five filter types.
    A byte depends on its left, upper and upper-left neighbours, so the pixels of one anti-diagonal x + y = d are independent: the image is
    rebuilt diagonal by diagonal, h + w - 1 NumPy steps in place of a Python step per byte (libpng picks Paeth for most lines of a
    photograph-like map; a 1242 x 375 KITTI map is 2.8 M bytes)."""
    lines = np.frombuffer(filtered, np.uint8).reshape(h, 1 + w * bpp)
    ftype = lines[:, 0].astype(np.int32)
    if ftype.max(initial=0) > 4:
        raise ValueError(f"PNG: unknown filter type {int(ftype.max())}")
    data = lines[:, 1:].reshape(h, w, bpp).astype(np.int32)
    out = np.zeros((h + 1, w + 1, bpp), np.int32)               # pixel (y, x) at out[y + 1, x + 1]; row 0 and column 0 are the zeros outside
    rows = np.arange(h)
    for d in range(h + w - 1):
        y = rows[max(0, d - w + 1):min(h, d + 1)]
        x = d - y
        a, b, c = out[y + 1, x], out[y, x + 1], out[y, x]       # left, up, upper left
        f = ftype[y][:, np.newaxis]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        pred = np.where(f == 1, a, np.where(f == 2, b, np.where(f == 3, (a + b) >> 1, np.where(f == 4, paeth, 0))))
        out[y + 1, x + 1] = (data[y, x] + pred) & 255
    return out[1:, 1:].astype(np.uint8)


def read_png16_rgb(path):
    """A non-interlaced 16-bit RGB PNG -> uint16 [H, W, 3].  (PIL hands 16-bit RGB back as 8 bits per channel, so this is read here, on
    zlib: colour type 2, bit depth 16, all five filter types.)  Anything else is refused by name."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, head = 8, [], None
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if head is None:
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, depth, colour, _, _, interlace = head
    if depth != 16 or colour != 2:
        raise ValueError(f"{path}: bit depth {depth}, colour type {colour}: a KITTI flow map is 16-bit RGB (bit depth 16, colour type 2)")
    if interlace != 0:
        raise ValueError(f"{path}: interlaced PNG (Adam7) is not supported")
    bpp, stride = 6, 6 * w
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (stride + 1):
        raise ValueError(f"{path}: {len(raw)} bytes of image data, expected {h * (stride + 1)}")
    return np.frombuffer(_unfilter(raw, h, w, bpp).tobytes(), ">u2").reshape(h, w, 3).astype(np.uint16)


def write_png16_rgb(path, rgb, filter_type=0):
    """uint16 [H, W, 3] -> a non-interlaced 16-bit RGB PNG, every scanline with PNG filter `filter_type` (0 .. 4)."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint16:
        raise ValueError(f"write_png16_rgb: need uint16 [H,W,3], got {rgb.dtype} {rgb.shape}")
    h, w = rgb.shape[:2]
    lines, prev = [], bytearray(6 * w)
    for y in range(h):
        row = bytearray(rgb[y].astype(">u2").tobytes())
        lines.append(bytes([filter_type]) + bytes(_filter_row(filter_type, row, prev, 6)))
        prev = row
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(b"".join(lines)))
                + _chunk(b"IEND", b""))


def read_kitti_flow(path):
    """KITTI flow PNG -> (flow [2,H,W] float32, valid [1,H,W] float32)."""
    rgb = read_png16_rgb(path)
    uv = (rgb[:, :, :2].astype(np.float32) - np.float32(2 ** 15)) / np.float32(64)      # exact: a 16-bit integer over a power of two
    return np.ascontiguousarray(uv.transpose(2, 0, 1)), (rgb[:, :, 2] != 0).astype(np.float32)[np.newaxis]


def write_kitti_flow(path, flow, valid=None, filter_type=0):
    """The writer that matches read_kitti_flow (fixtures): flow [2,H,W] in steps of 1 / 64 within +-512, valid [1,H,W] or [H,W] or None."""
    flow = np.asarray(flow, np.float64)
    q = np.rint(flow * 64.0 + 2 ** 15)
    if q.min() < 0 or q.max() > 65535:
        raise ValueError("write_kitti_flow: flow outside the format's range of -512 .. 511.98")
    v = np.ones(flow.shape[1:], bool) if valid is None else np.asarray(valid).reshape(flow.shape[1:]) != 0
    rgb = np.stack([q[0], q[1], v.astype(np.float64)], axis=-1).astype(np.uint16)
    rgb[~v, :2] = 0                                                                       # the devkit writes an invalid pixel as (0, 0, 0)
    write_png16_rgb(path, rgb, filter_type)


# ---- ground truth and lists --------------------------------------------------------------------------------------------------------
def _plane(a, what):
    a = np.asarray(a)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    if a.ndim == 3:                     # a colour mask image: any channel set
        a = a.any(axis=2)
    if a.ndim != 2:
        raise ValueError(f"{what}: expected a [H,W] mask, got {a.shape}")
    return (a != 0).astype(np.float32)[np.newaxis]


def read_mask(path):
    """A mask file -> [1,H,W] float32 of 0 / 1: .npy, or any image PIL reads (non-zero = set)."""
    if path.endswith(".npy"):
        return _plane(np.load(path), path)
    from PIL import Image
    return _plane(np.asarray(Image.open(path)), path)


def read_ground_truth(path, mask=None, mask_as="valid"):
    """-> (flow [2,H,W] float32, valid [1,H,W] float32 or None, occ [1,H,W] float32 or None) from a .flo, a .npz (`flow` as [2,H,W] or
    [H,W,2], optional `valid` / `occ`) or a KITTI flow .png; `mask`: a mask file read as `valid` or, with mask_as="occ", as `occ`."""
    if mask_as not in ("valid", "occ"):
        raise ValueError(f"mask_as: 'valid' or 'occ', got {mask_as!r}")
    valid = occ = None
    if path.endswith(".flo"):
        flow = flo.read_flo(path).transpose(2, 0, 1)
    elif path.endswith(".npz"):
        with np.load(path) as z:
            flow = np.asarray(z["flow"], np.float32)
            if flow.ndim != 3 or 2 not in (flow.shape[0], flow.shape[2]):
                raise ValueError(f"{path}: flow must be [2,H,W] or [H,W,2], got {flow.shape}")
            if flow.shape[2] == 2:                                                      # [H,W,2], as flo.write_flo reads a [2,H,2] array
                flow = flow.transpose(2, 0, 1)
            valid = _plane(z["valid"], path + ":valid") if "valid" in z else None
            occ = _plane(z["occ"], path + ":occ") if "occ" in z else None
    elif path.endswith(".png"):
        flow, valid = read_kitti_flow(path)
    else:
        raise ValueError(f"{path}: ground truth must be .flo, .npz or a KITTI flow .png")
    flow = np.ascontiguousarray(flow, np.float32)
    if mask is not None:
        m = read_mask(mask)
        if m.shape[1:] != flow.shape[1:]:
            raise ValueError(f"{mask}: mask {m.shape[1:]} does not match the flow {flow.shape[1:]}")
        if mask_as == "valid":
            valid = m if valid is None else valid * m
        else:
            occ = m
    return flow, valid, occ


def parse_list(lines):
    """List lines `img0 img1 gt [mask]` -> [(img0, img1, gt, mask or None)]; blank lines and lines starting with # are skipped."""
    out = []
    for no, line in enumerate(lines, 1):
        tok = line.split()
        if not tok or tok[0].startswith("#"):
            continue
        if len(tok) not in (3, 4):
            raise ValueError(f"list line {no}: expected `img0 img1 gt [mask]`, got {len(tok)} fields")
        out.append((tok[0], tok[1], tok[2], tok[3] if len(tok) == 4 else None))
    return out


# ---- the data-set loop -------------------------------------------------------------------------------------------------------------
def prefetched(items, depth):
    """Iterate `items` on a thread of its own that stays up to `depth` items ahead; its exception is raised here."""
    q, end = queue.Queue(maxsize=max(1, depth)), object()

    def run():
        try:
            for it in items:
                q.put(it)
            q.put(end)
        except BaseException as e:      # noqa: BLE001 -- surfaced on the consumer's thread
            q.put(e)

    threading.Thread(target=run, daemon=True).start()
    while True:
        it = q.get()
        if it is end:
            return
        if isinstance(it, BaseException):
            raise it
        yield it


def _stack(planes, shape, absent):
    """[n,1,H,W] from per-sample [1,H,W] masks; None when no sample has one, `absent` everywhere for a sample without where others have."""
    if all(p is None for p in planes):
        return None
    return np.stack([p if p is not None else np.full(shape, absent, np.float32) for p in planes])


def gather(total, parts):
    """parts: this rank's [(list indices, FlowMetrics)].  Over the process group (gloo: Python objects) every rank's parts go to rank 0,
    which returns the FlowMetrics of all `total` samples in list order; the other ranks return None."""
    from . import parallel
    mine = [(list(idx), m.rows) for idx, m in parts]
    if parallel.world() > 1:
        import torch.distributed as dist
        every = [None] * parallel.world() if parallel.rank() == 0 else None
        dist.gather_object(mine, every, dst=0)
        if parallel.rank() != 0:
            return None
        mine = [p for r in every for p in r]
    rows, seen = np.zeros((total, K), np.float64), np.zeros(total, bool)
    for idx, r in mine:
        rows[idx] = r
        seen[idx] = True
    if not seen.all():
        raise RuntimeError(f"evaluate.gather: no result for list entries {np.flatnonzero(~seen).tolist()}")
    return FlowMetrics(rows)


def gather_consistency(total, parts, alpha=(0.01, 0.5), beta=(0.01, 0.002)):
    """gather() for FlowConsistency: parts is this rank's [(list indices, FlowConsistency)]; rank 0 returns the FlowConsistency of all
    `total` samples in list order, the other ranks None."""
    from . import parallel
    mine = [(list(idx), c.rows_fw, c.rows_bw) for idx, c in parts]
    if parallel.world() > 1:
        import torch.distributed as dist
        every = [None] * parallel.world() if parallel.rank() == 0 else None
        dist.gather_object(mine, every, dst=0)
        if parallel.rank() != 0:
            return None
        mine = [p for r in every for p in r]
    fw, bw, seen = np.zeros((total, CONSISTENCY_K), np.float64), np.zeros((total, CONSISTENCY_K), np.float64), np.zeros(total, bool)
    for idx, rf, rb in mine:
        fw[idx], bw[idx] = rf, rb
        seen[idx] = True
    if not seen.all():
        raise RuntimeError(f"evaluate.gather_consistency: no result for list entries {np.flatnonzero(~seen).tolist()}")
    return FlowConsistency(fw, bw, alpha=alpha, beta=beta)


def evaluate(entries, groups_of, read_image, predict, metrics, batch=8, prefetch=2, mask_as="valid", on_group=None, occ_present=False):
    """Score a list.  entries: parse_list's tuples.  This rank takes its shard (parallel.shard), groups it into batches of at most `batch`
    consecutive pairs of equal image size (groups_of: scripts/run_flownet_many.py's), reads images and ground truth `prefetch` groups
    ahead, and for every group calls pred = predict(img0 [n,3,H,W], img1) and metrics(pred, gt, valid, occ) -> FlowMetrics (both given
    NumPy arrays; what predict returns is handed to metrics as it is).  on_group(entries, FlowMetrics) sees every group (the epe maps).
    With occ_present, metrics gets a fifth argument: per sample, whether its ground truth came with an occlusion mask (where some do and
    some do not, `occ` is 0 for those that do not).
    Returns gather()'s result: all samples in list order on rank 0, None on the other ranks."""
    from . import parallel
    mine = parallel.shard([e + (i,) for i, e in enumerate(entries)])

    def staged():
        for ents, i0, i1 in groups_of(mine, batch, read_image):
            gts = [read_ground_truth(e[2], e[3], mask_as) for e in ents]
            hw = gts[0][0].shape[1:]
            for e, g in zip(ents, gts):
                if g[0].shape[1:] != hw or tuple(i0.shape[2:]) != tuple(hw):
                    raise ValueError(f"{e[2]}: ground truth {g[0].shape[1:]} does not match the images {tuple(i0.shape[2:])}")
            yield (ents, i0, i1, np.stack([g[0] for g in gts]), _stack([g[1] for g in gts], (1,) + hw, 1.0),
                   _stack([g[2] for g in gts], (1,) + hw, 0.0), [g[2] is not None for g in gts])

    parts = []
    for ents, i0, i1, gt, valid, occ, has_occ in prefetched(staged(), prefetch):
        m = metrics(predict(i0, i1), gt, valid, occ, has_occ) if occ_present else metrics(predict(i0, i1), gt, valid, occ)
        if len(m) != len(ents):
            raise RuntimeError(f"evaluate: {len(m)} rows for {len(ents)} samples")
        if on_group is not None:
            on_group(ents, m)
        parts.append(([e[4] for e in ents], m))
    return gather(len(entries), parts)
