"""flownet2_amd: MI355X (gfx950) implementation of the FlowNet2 hot path of lmb-freiburg/flownet2.

csrc/      hand-written HIP kernels + the C ABI (include/flownet2_hip.h) -> libflownet2_hip.so
_lib/ops   ctypes binding (no fallback: a missing library raises)
layers     host-side mirror of the reference's Caffe Layer<Dtype> / LayerRegistry interface
functional torch.autograd glue,  nets: FlowNetC/S graphs,  flo: .flo I/O
solver     SolverParameter, Solver (SGDSolver / AdamSolver, get_solver) and CaffeOptimizer on the one-launch HIP update
LpqSchedule  the p / q episodes of LpqLoss (lpq_schedule.py)
evaluate   FlowMetrics (the rows of the metrics kernel, summary()), ground-truth readers incl. the KITTI flow PNG, the data-set loop
flow_consistency  forward-backward consistency of two flows -> FlowConsistency (occlusion masks, rows, summary()) in one launch
visualize  flow_to_color (Middlebury colour coding) and flow_error_map (KITTI-style error image) on fused kernels, color_wheel, write_png
unsupervised_loss  photometric + smoothness training loss without ground truth, one fused pass per direction of differentiation;
            unsupervised_loss_report -> UnsupLoss (rows, summary())
census_loss  the census data term of UnFlow (soft Hamming distance of ternary census signatures over a patch) on fused kernels: unchanged
            by an additive change of brightness; unsupervised_loss(data_term="census") uses it; census_loss_report -> CensusLoss
flow_splat  forward warping (summation / average / linear / softmax splatting) with gradients, the same bits from run to run;
            flow_splat_report -> FlowSplat; flow_range_occlusion (range-map occlusion planes); flow_interpolate (the frame between two frames)
flow_track  points carried through a flow sequence in one launch -> FlowTracks (trajectories, long_range_flow()); flow_track_reseed, flow_track_grid
"""
from . import _lib  # noqa: F401
from ._lib import Fn2Error, version  # noqa: F401

_SOLVER_EXPORTS = ("SolverParameter", "Solver", "SGDSolver", "AdamSolver", "get_solver", "CaffeOptimizer")
__all__ = ["Fn2Error", "version", "LpqSchedule", "flow_consistency", "FlowConsistency", "flow_to_color", "flow_error_map", "flow_track",
           "flow_track_reseed", "flow_track_grid", "FlowTracks", "unsupervised_loss", "unsupervised_loss_report", "UnsupLoss", "census_loss",
           "census_loss_report", "CensusLoss", "flow_splat", "flow_splat_report", "flow_range_occlusion", "flow_interpolate", "FlowSplat",
           *_SOLVER_EXPORTS]


def __getattr__(name):
    # the solver's names, resolved on first use: importing the package alone still loads neither torch nor the operator modules
    if name in _SOLVER_EXPORTS:
        from . import solver
        return getattr(solver, name)
    if name == "LpqSchedule":
        from .lpq_schedule import LpqSchedule
        return LpqSchedule
    if name == "flow_consistency":
        from .functional import flow_consistency
        return flow_consistency
    if name in ("flow_to_color", "flow_error_map", "flow_track", "flow_track_reseed", "flow_track_grid", "unsupervised_loss",
                "unsupervised_loss_report", "census_loss", "census_loss_report", "flow_splat", "flow_splat_report", "flow_range_occlusion",
                "flow_interpolate"):
        from . import functional
        return getattr(functional, name)
    if name == "FlowConsistency":
        from .evaluate import FlowConsistency
        return FlowConsistency
    if name == "FlowTracks":
        from .evaluate import FlowTracks
        return FlowTracks
    if name == "UnsupLoss":
        from .evaluate import UnsupLoss
        return UnsupLoss
    if name == "CensusLoss":
        from .evaluate import CensusLoss
        return CensusLoss
    if name == "FlowSplat":
        from .evaluate import FlowSplat
        return FlowSplat
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
