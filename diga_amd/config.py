"""Explicit configuration of the step driver and of the layers' path choices (round 6).

Until round 5 the stream policy and a dozen path switches were steered through `os.environ` AT RUN TIME (the trainer set and
popped DIGA_TEACHER_STREAM / DIGA_WGRAD_STREAM around a graph capture, ddp.init_from_env wrote them for gloo, bench.py flipped
them around timed code): process-global, not thread-safe, invisible in a trainer's signature.  Now:

  * `StepConfig` holds every switch as a typed field;
  * environment variables are read ONCE, at import, into `DEFAULTS` (so `DIGA_*=... python train.py` keeps working as a way to
    set defaults) -- nothing in the package reads or writes `os.environ` after that (ddp.init_from_env's MASTER_* defaults aside);
  * `DigaTrainer(config=...)` owns a config and runs every step under `use(cfg)`; the layers (DigaConv2d, the norm layers, the
    bottleneck wiring, GradReducer) read `active()` at call time;
  * tests and A/B runs change fields (`with override(c4_overlap=0): ...`, `dataclasses.replace(DEFAULTS, ...)`) instead of the
    environment.

A config is plain data: copying one (`dataclasses.replace`) never touches a trainer that holds the original.
"""
import contextlib
import dataclasses
import os
from dataclasses import dataclass


def _flag(name, default):
    v = os.environ.get(name)
    if v is None:
        return default
    return v not in ("0", "", "false", "False")


@dataclass
class StepConfig:
    # ---- streams of the step driver (diga_amd/train_step.py)
    teacher_stream: bool = True          # teacher forward(s) on a second HIP stream next to the student's forward
    teacher_offset: str = "layer1"       # the student stage behind which the teacher is enqueued ("" / "0": both at once)
    wgrad_stream: bool = True            # weight gradients on a side stream next to the backward-data / BatchNorm chain
    wgrad_hold: int = 4                  # ... whose inputs are held for this many layers and released behind an event (0: record_stream)
    wgrad_hold_batch: int = 4            # ... that many at a time (one device-side wait per batch)
    c4_overlap: int = 2                  # self-training step: 0 one backward pass; 1 cross-mixed fwd/bwd on a third stream; 2 the whole target branch
    c4_overlap_gloo: bool = False        # keep the overlapped forms under the gloo smoke-test backend (slow there, not wrong)
    step_graph: bool = False             # replay the static part of the warm-up step from a HIP graph (launch-bound configurations)
    graph_fork_teacher: bool = True      # ... with the teacher's forward as a forked branch of the captured graph
    graph_fork_wgrad: bool = True        # ... and the weight gradients as forked branches
    centroid_exchange: str = "allgather"  # N > 1: "allgather" (exact) or "allreduce" (BASELINE configs[3]'s approximate exchange)
    # ---- convolution arithmetic and path choices (diga_amd/model/conv.py)
    conv_math: int = 0                   # 0 exact fp32 (matrix cores, Winograd for stride-1 3x3), 1 split bf16 (three bf16 MFMAs per product), 2 bf16x6 (pointwise layers on three bf16 planes, fp32-equivalent; the rest as 0)
    x6_split: str = "pass"               # bf16x6 operands: "pass" split by an elementwise pass into triplet buffers, "loader" split by the GEMMs' loader waves straight from the fp32 tensors (bit-identical; no triplet buffers, channel slices not copied)
    x6_winograd: bool = False            # conv_math 2 only: the Winograd-domain GEMMs of the stride-1 3x3 layers on bf16x6 as well (loader form, whatever x6_split says; the transforms stay fp32)
    x6_taps: bool = False                # conv_math 2 only: every multi-tap convolution that would run on the direct fp32 kernels (Cin % 32 == 0, no folded options), and the stem's im2col GEMM, on bf16x6 as well (loader form, whatever x6_split says)
    x6_opts: bool = False                # conv_math 2 only: lifts the "no folded options" exclusion of x6_taps and x6_winograd and nothing else -- a call with a diga_conv_options_t (reflection padding / nearest upsampling / tanh folded into the kernel: the frozen translator) is planned by the same rules as one without: multi-tap calls on the multi-tap bf16x6 kernels (with x6_taps), the products of the reflect-padded Winograd layers on bf16x6 (with x6_winograd); pointwise calls with options stay exact fp32
    x6_window: bool = False              # conv_math 2 with x6_taps only: a stride-1 multi-tap forward without statistics and without an epilogue that diga_conv_window_bf16x6_plan admits runs on the window form (diga_conv_window_bf16x6_f32in: the tile's input window split into LDS once, all taps walked from there); with folded options only next to x6_opts; everything else keeps its path; read per call
    x6_up2: bool = False                 # conv_math 2 with x6_taps, x6_opts and x6_window only: a window-form forward of a 2x nearest-upsampled input that diga_conv_up2_bf16x6_plan admits runs its interior tiles on phase-collapsed weights (diga_conv_up2_bf16x6_f32in: four stride-1 convolutions of the SOURCE image, one per output parity, R' x S' summed taps instead of R x S) and only the ring of border tiles on the window walk; everything else keeps its path; read per call
    x6_wgrad_tile: str = "wide"          # conv_math 2 only: the loader-form bf16x6 weight gradient ("x6ls" / "x6rs") on "wide" = the one 256 x 128 tile, or "fit" = the tile diga_wgrad_bf16x6_tile picks for the layer (64x64 / 64x128 / 128x128 / 256x64 for the narrow layers, another split-K plan; 256 x 128 layers unchanged); read per call
    winograd: bool = True
    winograd_ratio: float = 0.62
    winograd_default_max_tile: int = 6
    winograd_max_tile: int = 6           # 2 keeps every layer on F(2x2,3x3) (set_conv_math(0, exact=True))
    winograd_keep_v: bool = True         # keep the forward's input transform for the weight gradient
    winograd_stats: bool = True          # BatchNorm statistics from the Winograd output transform
    keep_v_max_gb: float = 8.0           # per layer
    keep_v_min_device_gb: float = 160.0
    conv_twin: str = "3"                 # split-bf16 twin kernels: "0" off, "1" every eligible conv, "3" multi-tap / shared inputs
    twin_only: bool = True               # producers write the split twin INSTEAD of the fp32 tensor where every reader takes twins
    twin_conv3: str = "1"
    # ---- norm layers / bottleneck wiring (diga_amd/model/norm.py, seg_model_noaux.py)
    relu_bits: bool = True               # ReLU masks as bit planes instead of reading the activated tensor in backward
    fuse_bwd: bool = True                # residual-junction add + ReLU mask + BN-backward reduce in the backward-data epilogue
    junction_chain: bool = True
    fold_downsample_bn: bool = True      # the downsample BatchNorm's apply pass inside the junction relu(bn3(c3) + skip) that alone reads it
    fold_eval_bn: bool = False           # eval-mode BatchNorm (+ skip, + ReLU) of the trunk inside the epilogue of the fp32 conv in front of it (bit-identical; offline passes)
    fold_eval_bn_x6: bool = False        # ... and, under conv_math 2, inside the bf16x6 kernels as well: the pointwise layers' drain and, with x6_winograd, the Winograd output transform behind the bf16x6 products (means something only with fold_eval_bn)
    # ---- data parallelism (diga_amd/ddp.py)
    ddp_bucket_mb: int = 25
    ddp_grad_views: bool = True          # gradients live in the all-reduce buckets
    ddp_overlap: bool = True             # hook-driven bucket launches inside backward
    ddp_single_rank: bool = False        # run the reducer (hooks, views, collectives) even at world size 1 (the 1-rank RCCL test)
    # ---- MiT / SegFormer student
    mit_loss_scale: float = 1024.0

    @classmethod
    def from_env(cls):
        e = os.environ.get
        c = cls()
        c.teacher_stream = _flag("DIGA_TEACHER_STREAM", c.teacher_stream)
        c.teacher_offset = e("DIGA_TEACHER_OFFSET", c.teacher_offset)
        c.wgrad_stream = _flag("DIGA_WGRAD_STREAM", c.wgrad_stream)
        c.wgrad_hold = int(e("DIGA_WGRAD_HOLD", c.wgrad_hold))
        c.wgrad_hold_batch = int(e("DIGA_WGRAD_HOLD_BATCH", c.wgrad_hold_batch))
        c.c4_overlap = int(e("DIGA_C4_OVERLAP", c.c4_overlap))
        c.c4_overlap_gloo = _flag("DIGA_C4_OVERLAP_GLOO", c.c4_overlap_gloo)
        c.step_graph = _flag("DIGA_STEP_GRAPH", c.step_graph)
        c.graph_fork_teacher = _flag("DIGA_GRAPH_FORK_TEACHER", c.graph_fork_teacher)
        c.graph_fork_wgrad = _flag("DIGA_GRAPH_FORK_WGRAD", c.graph_fork_wgrad)
        c.centroid_exchange = e("DIGA_CENTROID_EXCHANGE", c.centroid_exchange)
        c.conv_math = {"bf16x3": 1, "1": 1, "bf16x6": 2, "2": 2}.get(e("DIGA_CONV_MATH", ""), 0)
        c.x6_split = e("DIGA_X6_SPLIT", c.x6_split)
        c.x6_winograd = _flag("DIGA_X6_WINOGRAD", c.x6_winograd)
        c.x6_taps = _flag("DIGA_X6_TAPS", c.x6_taps)
        c.x6_opts = _flag("DIGA_X6_OPTS", c.x6_opts)
        c.x6_window = _flag("DIGA_X6_WINDOW", c.x6_window)
        c.x6_up2 = _flag("DIGA_X6_UP2", c.x6_up2)
        c.x6_wgrad_tile = e("DIGA_X6_WGRAD_TILE", c.x6_wgrad_tile)
        c.winograd = _flag("DIGA_CONV_WINOGRAD", c.winograd)
        c.winograd_ratio = float(e("DIGA_CONV_WINOGRAD_RATIO", c.winograd_ratio))
        c.winograd_default_max_tile = c.winograd_max_tile = int(e("DIGA_CONV_WINOGRAD_TILE", c.winograd_default_max_tile))
        c.winograd_keep_v = _flag("DIGA_WINOGRAD_KEEP_V", c.winograd_keep_v)
        c.winograd_stats = _flag("DIGA_WINOGRAD_STATS", c.winograd_stats)
        c.keep_v_max_gb = float(e("DIGA_WINOGRAD_KEEP_V_MAX_GB", c.keep_v_max_gb))
        c.keep_v_min_device_gb = float(e("DIGA_WINOGRAD_KEEP_V_MIN_DEVICE_GB", c.keep_v_min_device_gb))
        c.conv_twin = e("DIGA_CONV_TWIN", c.conv_twin)
        c.twin_only = _flag("DIGA_TWIN_ONLY", c.twin_only)
        c.twin_conv3 = e("DIGA_TWIN_CONV3", c.twin_conv3)
        c.relu_bits = _flag("DIGA_RELU_BITS", c.relu_bits)
        c.fuse_bwd = _flag("DIGA_FUSE_BWD", c.fuse_bwd)
        c.junction_chain = _flag("DIGA_JUNCTION_CHAIN", c.junction_chain)
        c.fold_downsample_bn = _flag("DIGA_FOLD_DOWNSAMPLE_BN", c.fold_downsample_bn)
        c.fold_eval_bn = _flag("DIGA_FOLD_EVAL_BN", c.fold_eval_bn)
        c.fold_eval_bn_x6 = _flag("DIGA_FOLD_EVAL_BN_X6", c.fold_eval_bn_x6)
        c.ddp_bucket_mb = int(e("DIGA_DDP_BUCKET_MB", c.ddp_bucket_mb))
        c.ddp_grad_views = _flag("DIGA_DDP_GRAD_VIEWS", c.ddp_grad_views)
        c.ddp_overlap = _flag("DIGA_DDP_OVERLAP", c.ddp_overlap)
        c.ddp_single_rank = _flag("DIGA_DDP_SINGLE_RANK", c.ddp_single_rank)
        c.mit_loss_scale = float(e("DIGA_MIT_LOSS_SCALE", c.mit_loss_scale))
        c.validate()
        return c

    def validate(self):
        if self.centroid_exchange not in ("allgather", "allreduce"):
            raise ValueError(f"centroid_exchange must be 'allgather' or 'allreduce', not {self.centroid_exchange!r}")
        if self.c4_overlap not in (0, 1, 2):
            raise ValueError(f"c4_overlap must be 0, 1 or 2, not {self.c4_overlap!r}")
        if self.wgrad_hold < 0:
            raise ValueError(f"wgrad_hold must be >= 0, not {self.wgrad_hold!r}")
        if self.conv_math not in (0, 1, 2):
            raise ValueError(f"conv_math must be 0 (fp32), 1 (split bf16) or 2 (bf16x6), not {self.conv_math!r}")
        if self.x6_split not in ("pass", "loader"):
            raise ValueError(f"x6_split must be 'pass' or 'loader', not {self.x6_split!r}")
        if not isinstance(self.x6_winograd, bool):
            raise ValueError(f"x6_winograd must be a bool, not {self.x6_winograd!r}")
        if not isinstance(self.x6_taps, bool):
            raise ValueError(f"x6_taps must be a bool, not {self.x6_taps!r}")
        if not isinstance(self.x6_opts, bool):
            raise ValueError(f"x6_opts must be a bool, not {self.x6_opts!r}")
        if not isinstance(self.x6_window, bool):
            raise ValueError(f"x6_window must be a bool, not {self.x6_window!r}")
        if not isinstance(self.x6_up2, bool):
            raise ValueError(f"x6_up2 must be a bool, not {self.x6_up2!r}")
        if self.x6_wgrad_tile not in ("wide", "fit"):
            raise ValueError(f"x6_wgrad_tile must be 'wide' or 'fit', not {self.x6_wgrad_tile!r}")
        if not isinstance(self.fold_eval_bn, bool):
            raise ValueError(f"fold_eval_bn must be a bool, not {self.fold_eval_bn!r}")
        if not isinstance(self.fold_eval_bn_x6, bool):
            raise ValueError(f"fold_eval_bn_x6 must be a bool, not {self.fold_eval_bn_x6!r}")
        if self.winograd_max_tile not in (2, 4, 6):
            raise ValueError(f"winograd_max_tile must be 2, 4 or 6, not {self.winograd_max_tile!r}")
        return self

    def replace(self, **fields):
        return dataclasses.replace(self, **fields).validate()

    def serial_streams(self):
        """A copy with every side stream off (kernel timing, graph capture on one stream, the gloo smoke-test backend)."""
        return self.replace(teacher_stream=False, wgrad_stream=False, c4_overlap=0)


DEFAULTS = StepConfig.from_env()       # the ONE read of the environment
_stack = [DEFAULTS]


def active():
    """The configuration in force: the innermost `use(...)`, else the process defaults."""
    return _stack[-1]


@contextlib.contextmanager
def use(cfg):
    """Run the body under `cfg` (DigaTrainer wraps every step in this).  Not re-entrant across threads by design: one process
    drives one GPU from one thread."""
    _stack.append(cfg)
    try:
        yield cfg
    finally:
        _stack.pop()


@contextlib.contextmanager
def override(**fields):
    """`with override(c4_overlap=0): ...` -- the active configuration with some fields replaced."""
    with use(active().replace(**fields)) as cfg:
        yield cfg
