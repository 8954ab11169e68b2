"""ctypes binding of libgode.so (include/gode.h).  There is NO fallback: if the library is missing or a call
fails, a RuntimeError is raised -- the product path never runs on anything but the HIP kernels."""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgode.so")

i32, i64, f32, ptr = C.c_int32, C.c_int64, C.c_float, C.c_void_p
cint, u32, u64 = C.c_int, C.c_uint32, C.c_uint64

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH_OUT = 0, 1, 2, 3
ACT_TANH, ACT_SIGMOID = 4, 5   # gode_fc_act / gode_fc_act_bwd only
ACT_LRELU01 = 6                # LeakyReLU(0.1): the convolution stack's ops (not gode_fc_act / gode_cbn_*)
EPI_RAW, EPI_TANH = 0, 1
FPROP, DGRAD = 0, 1
PACK_BORDER = 0x100          # or'ed into a pack's dir: the pack an IgemmOp with border=1 / 2 reads
OP_IGEMM, OP_WGRAD, OP_BN_FINALIZE, OP_BN_BWD, OP_ODE_FWD, OP_ODE_BWD, OP_BCE, OP_ADAM, OP_PACK = range(1, 10)
OP_ODERNN_FWD, OP_ODERNN_BWD, OP_BN_APPLY, OP_COL2IM = 10, 11, 12, 13
OP_SDE_FWD, OP_SDE_BWD = 14, 15
OP_CDE_FWD, OP_CDE_BWD = 16, 17
OP_WGAN = 18
OP_GRU_FWD, OP_GRU_BWD = 19, 20
OP_DNOISE = 21
OP_CATEG, OP_CE = 22, 23
OP_CHSTATS, OP_CBN_EMBED, OP_CBN_EMBED_BWD, OP_CBN_APPLY, OP_CBN_BWD, OP_GRES_OUT, OP_GRES_OUT_BWD, OP_SN_FWD, OP_SN_BWD = range(24, 33)
OP_FC_ACT, OP_FC_ACT_BWD, OP_BCE_PROB = 33, 34, 35
OP_BCE_T = 36
OP_RESIZE_U8, OP_CLIP_GATHER = 37, 38
OP_BN_RUNNING = 39
OP_ROT_CLIPS = 40
OP_VIDEO_GRID = 41
OP_LATENT_DRAW = 42
OP_DIFFAUG = 43
BN_RUNNING_MAX = 8            # GODE_BN_RUNNING_MAX: the layers one gode_bn_running launch takes
RESIZE_MAX_TAPS = 32          # GODE_RESIZE_MAX_TAPS: the longest tap row gode_resize_u8 takes
ROT_MIN_SIZE, ROT_MAX_SIZE = 4, 64   # the image heights and widths gode_rot_clips takes
REC_ADAM_NOISE = -1          # gode_sizeof index of the gode_adam_noise_tensor table record
ODE_NPARAM = 2672
ODERNN_NPARAM = 2176
SDE_NPARAM = 3216
CDE_NPARAM = 7536
CDE_MAX_N = 4096
GRU_NPARAM = 1632
SN_BWD_BLOCKS = 64
# `method` of gode_ode_fwd_op / gode_ode_bwd_op (include/gode.h), by torchdiffeq's solver name
ODE_METHODS = {"rk4": 0, "dopri5": 1, "euler": 2, "midpoint": 3}
# `rhs` of the same ops: the right-hand side the fixed-grid kernels integrate.  "mlp": f(y) = W2 tanh(W1 y + b1) + b2
# (models/mocogan_ode.py's ODEFunc); "tanh": f(y) = tanh(W1 y + b1) (models/mocogan_mnist.py's), W2 / b2 unused
ODE_RHS = {"mlp": 0, "tanh": 1}
ODE_RHS_TANH_NPARAM = 2400     # rhs 1: the gradient block ends behind b1 (the first 2400 floats of the ODE_NPARAM layout)


def ode_method_code(name):
    """torchdiffeq solver name -> the ops' `method` code; any solver libgode has no kernel for is an error."""
    try:
        return ODE_METHODS[name]
    except (KeyError, TypeError):
        raise NotImplementedError(f"ode_method {name!r}: libgode implements " + ", ".join(repr(k) for k in ODE_METHODS)
                                  + " ('rk4' is the reference's call)") from None


def ode_rhs_code(name):
    """Right-hand side name -> the ops' `rhs` code."""
    return ODE_RHS[name]


class ConvGeom(C.Structure):
    _fields_ = [(n, i32) for n in "N Ci Co Di Hi Wi Do Ho Wo kd kh kw sd sh sw pd ph pw".split()]

    def key(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


class _Op(C.Structure):
    """An op of gode_run (a GODE_OPS row of gode.h): a subclass names its kind and its `int FN(const op*, stream)` entry
    point once; _STRUCTS, the prototypes, EXPORTS and run_one's dispatch all follow from the subclasses."""


class IgemmOp(_Op):
    _fields_ = [("g", ConvGeom), ("dir", i32), ("act", i32), ("epilogue", i32), ("tile", i32), ("src", ptr),
                ("wpack", ptr), ("out", ptr), ("scale", ptr), ("shift", ptr), ("stats", ptr), ("gs", i64 * 5),
                ("work", ptr), ("groups", i32), ("border", i32)]
    KIND, FN = OP_IGEMM, "gode_igemm"


class WgradOp(_Op):
    _fields_ = [("g", ConvGeom), ("act", i32), ("xform_on_y", i32), ("splits", i32), ("accumulate", i32),
                ("x", ptr), ("y", ptr), ("scale", ptr), ("shift", ptr), ("work", ptr), ("dw", ptr),
                ("co_perm", ptr), ("co_canon", i64), ("xs", i64 * 5)]
    KIND, FN = OP_WGRAD, "gode_wgrad"


class BnFinalizeOp(_Op):
    _fields_ = [("stats", ptr), ("rows", i32), ("ncols", i32), ("C", i32), ("count", i64), ("gamma", ptr),
                ("beta", ptr), ("running_mean", ptr), ("running_var", ptr), ("num_batches_tracked", ptr),
                ("mean", ptr), ("invstd", ptr), ("scale", ptr), ("shift", ptr), ("momentum", f32), ("eps", f32),
                ("training", i32), ("pad_", i32), ("groups", i32), ("rows0", i32), ("nseg", i32), ("order", i32),
                ("count1", i64), ("seg", i32 * 24), ("stats1", ptr), ("rows1", i32), ("pad3_", i32), ("batch_var", ptr)]
    KIND, FN = OP_BN_FINALIZE, "gode_bn_finalize"


class BnRunningLayer(C.Structure):
    _fields_ = [("mean", ptr), ("var", ptr), ("running_mean", ptr), ("running_var", ptr), ("num_batches_tracked", ptr),
                ("C", i32), ("pad_", i32)]


class BnRunningOp(_Op):
    _fields_ = [("layer", BnRunningLayer * BN_RUNNING_MAX), ("n", i32), ("momentum", f32)]
    KIND, FN = OP_BN_RUNNING, "gode_bn_running"


class BnBwdOp(_Op):
    _fields_ = [("g", ptr), ("y", ptr), ("M", i64), ("C", i32), ("act", i32), ("gamma", ptr), ("mean", ptr),
                ("invstd", ptr), ("scale", ptr), ("shift", ptr), ("dgamma", ptr), ("dbeta", ptr), ("work", ptr),
                ("accumulate", i32), ("eval_mode", i32), ("gin", ptr), ("groups", i32), ("pad2_", i32), ("M0", i64),
                ("r1_s", ptr), ("r1_w", ptr), ("r1_H", i32), ("r1_W", i32), ("r1_h", i32), ("r1_wd", i32), ("r1_off", i32),
                ("pad3_", i32)]
    KIND, FN = OP_BN_BWD, "gode_bn_bwd"


class OdeParams(C.Structure):
    _fields_ = [(n, ptr) for n in "Wa ba Wb bb W1 b1 W2 b2".split()]


class OdeFwdOp(_Op):
    _fields_ = [("p", OdeParams), ("x", ptr), ("content", ptr), ("dt", ptr), ("sel_t", ptr), ("z", ptr),
                ("traj", ptr), ("N", i32), ("T", i32), ("substeps", i32), ("prenet", i32), ("zcols", i32), ("G", i32),
                ("grid_dt", ptr), ("emit_at", ptr), ("emit_w", ptr), ("method", i32), ("rhs", i32), ("rtol", f32),
                ("atol", f32), ("tout", ptr), ("nsteps", ptr), ("sync", ptr)]
    KIND, FN = OP_ODE_FWD, "gode_ode_fwd"


class OdeBwdOp(_Op):
    _fields_ = [("p", OdeParams), ("x", ptr), ("traj", ptr), ("dt", ptr), ("sel_t", ptr), ("gz", ptr),
                ("work", ptr), ("grads", ptr), ("N", i32), ("T", i32), ("substeps", i32), ("prenet", i32),
                ("accumulate", i32), ("zcols", i32), ("bstep_off", ptr), ("bstep_dt", ptr), ("method", i32),
                ("rhs", i32), ("rtol", f32), ("atol", f32), ("tout", ptr), ("nsteps", ptr), ("sync", ptr),
                ("backprop", i32), ("G", i32), ("grid_dt", ptr), ("emit_at", ptr), ("emit_w", ptr), ("ysteps", ptr)]
    KIND, FN = OP_ODE_BWD, "gode_ode_bwd"


class OdeRnnParams(C.Structure):
    _fields_ = [(n, ptr) for n in "W1 b1 W2 b2 Wih Whh bih bhh".split()]


class OdeRnnFwdOp(_Op):
    _fields_ = [("p", OdeRnnParams), ("noise", ptr), ("content", ptr), ("sel_t", ptr), ("z", ptr), ("hs", ptr),
                ("hp", ptr), ("nsteps", ptr), ("N", i32), ("T", i32), ("rtol", f32), ("atol", f32), ("zcols", i32),
                ("pad_", i32), ("sync", ptr)]
    KIND, FN = OP_ODERNN_FWD, "gode_odernn_fwd"


class OdeRnnBwdOp(_Op):
    _fields_ = [("p", OdeRnnParams), ("noise", ptr), ("hp", ptr), ("sel_t", ptr), ("gz", ptr), ("work", ptr),
                ("grads", ptr), ("N", i32), ("T", i32), ("substeps", i32), ("accumulate", i32), ("zcols", i32),
                ("pad_", i32), ("rtol", f32), ("atol", f32), ("sync", ptr), ("nsteps", ptr)]
    KIND, FN = OP_ODERNN_BWD, "gode_odernn_bwd"


class SdeParams(C.Structure):
    _fields_ = [(n, ptr) for n in "Wa ba Wb bb Wf1 bf1 Wf2 bf2 Wg1 bg1 Wg2 bg2".split()]


class SdeFwdOp(_Op):
    _fields_ = [("p", SdeParams), ("x", ptr), ("content", ptr), ("sel_t", ptr), ("dt", ptr), ("sqrt_dt", ptr),
                ("emit_at", ptr), ("emit_w0", ptr), ("emit_w1", ptr), ("z", ptr), ("states", ptr), ("N", i32),
                ("T", i32), ("S", i32), ("prenet", i32), ("zcols", i32), ("pad_", i32)]
    KIND, FN = OP_SDE_FWD, "gode_sde_fwd"


class SdeBwdOp(_Op):
    _fields_ = [("p", SdeParams), ("x", ptr), ("states", ptr), ("sel_t", ptr), ("dt", ptr), ("sqrt_dt", ptr),
                ("emit_at", ptr), ("emit_w0", ptr), ("emit_w1", ptr), ("gz", ptr), ("work", ptr), ("grads", ptr),
                ("N", i32), ("T", i32), ("S", i32), ("prenet", i32), ("accumulate", i32), ("zcols", i32)]
    KIND, FN = OP_SDE_BWD, "gode_sde_bwd"


class CdeParams(C.Structure):
    _fields_ = [(n, ptr) for n in "Wa ba Wb bb W1 b1 W2 b2".split()]


class CdeFwdOp(_Op):
    _fields_ = [("p", CdeParams), ("x", ptr), ("tslope", ptr), ("content", ptr), ("sel_t", ptr), ("z", ptr),
                ("states", ptr), ("sched", ptr), ("counts", ptr), ("sync", ptr), ("N", i32), ("T", i32),
                ("S_cap", i32), ("zcols", i32), ("rtol", f32), ("atol", f32)]
    KIND, FN = OP_CDE_FWD, "gode_cde_fwd"


class CdeBwdOp(_Op):
    _fields_ = [("p", CdeParams), ("x", ptr), ("tslope", ptr), ("sel_t", ptr), ("states", ptr), ("sched", ptr),
                ("counts", ptr), ("gz", ptr), ("work", ptr), ("grads", ptr), ("N", i32), ("T", i32), ("S_cap", i32),
                ("accumulate", i32), ("zcols", i32), ("pad_", i32)]
    KIND, FN = OP_CDE_BWD, "gode_cde_bwd"


class GruParams(C.Structure):
    _fields_ = [(n, ptr) for n in "Wih Whh bih bhh".split()]


class GruFwdOp(_Op):
    _fields_ = [("p", GruParams), ("noise", ptr), ("content", ptr), ("sel_t", ptr), ("z", ptr), ("hs", ptr), ("N", i32),
                ("T", i32), ("zcols", i32), ("pad_", i32)]
    KIND, FN = OP_GRU_FWD, "gode_gru_fwd"


class GruBwdOp(_Op):
    _fields_ = [("p", GruParams), ("noise", ptr), ("hs", ptr), ("sel_t", ptr), ("gz", ptr), ("work", ptr), ("grads", ptr),
                ("N", i32), ("T", i32), ("accumulate", i32), ("zcols", i32)]
    KIND, FN = OP_GRU_BWD, "gode_gru_bwd"


class BnApplyOp(_Op):
    _fields_ = [("y", ptr), ("out", ptr), ("scale", ptr), ("shift", ptr), ("M", i64), ("C", i32), ("act", i32),
                ("M0", i64)]
    KIND, FN = OP_BN_APPLY, "gode_bn_apply"


class DnoiseOp(_Op):
    _fields_ = [("x", ptr), ("out", ptr), ("scale", ptr), ("shift", ptr), ("call_dev", ptr), ("M", i64), ("C", i32),
                ("act", i32), ("M0", i64), ("e_off", i64), ("xs", i64 * 5), ("N", i32), ("D", i32), ("H", i32), ("W", i32),
                ("seed", i64), ("stream", i32), ("layer", i32), ("call", i32), ("sigma", f32)]
    KIND, FN = OP_DNOISE, "gode_dnoise"


class Col2imOp(_Op):
    _fields_ = [("cols", ptr), ("out", ptr)] + [(n, i32) for n in "N Hi Wi Ho Wo C kh kw sh sw ph pw epilogue pad_ Di Do kd sd pd pad2_".split()]
    KIND, FN = OP_COL2IM, "gode_col2im"


class BceOp(_Op):
    _fields_ = [("logits", ptr), ("grad", ptr), ("loss", ptr), ("n", i64), ("target", f32), ("gscale", f32),
                ("accumulate", i32), ("stride", i32)]
    KIND, FN = OP_BCE, "gode_bce_logits"


class CategOp(_Op):
    _fields_ = [("cls", ptr), ("z", ptr), ("labels_out", ptr), ("n_traj", i32), ("rows_per", i32), ("C", i32),
                ("zcols", i32), ("col0", i32), ("pad_", i32)]
    KIND, FN = OP_CATEG, "gode_categ_onehot"


class CeOp(_Op):
    _fields_ = [("logits", ptr), ("labels", ptr), ("grad", ptr), ("loss", ptr), ("B", i32), ("n_lab", i32), ("C", i32),
                ("ld", i32), ("gld", i32), ("gscale", f32), ("accumulate", i32), ("rows_per_label", i32)]
    KIND, FN = OP_CE, "gode_ce_logits"


class WganOp(_Op):
    _fields_ = [("fake", ptr), ("real", ptr), ("grad_fake", ptr), ("grad_real", ptr), ("loss", ptr), ("n", i64),
                ("sign", f32), ("gscale", f32), ("reduction", i32), ("accumulate", i32)]
    KIND, FN = OP_WGAN, "gode_wgan_logits"


class ChstatsOp(_Op):
    _fields_ = [("x", ptr), ("stats", ptr), ("xs", i64 * 4), ("N", i32), ("H", i32), ("W", i32), ("C", i32), ("rows", i32),
                ("pad_", i32)]
    KIND, FN = OP_CHSTATS, "gode_chstats"


class CbnEmbedOp(_Op):
    _fields_ = [("cond", ptr), ("W", ptr), ("b", ptr), ("gb", ptr), ("N", i32), ("K", i32), ("C2", i32), ("pad_", i32)]
    KIND, FN = OP_CBN_EMBED, "gode_cbn_embed"


class CbnEmbedBwdOp(_Op):
    _fields_ = [("cond", ptr), ("W", ptr), ("dgb", ptr), ("dW", ptr), ("db", ptr), ("dcond", ptr), ("N", i32), ("K", i32),
                ("C2", i32), ("pad_", i32)]
    KIND, FN = OP_CBN_EMBED_BWD, "gode_cbn_embed_bwd"


class CbnApplyOp(_Op):
    _fields_ = [("src", ptr), ("bias", ptr), ("mean", ptr), ("invstd", ptr), ("gb", ptr), ("out", ptr), ("ss", i64 * 4),
                ("N", i32), ("H", i32), ("W", i32), ("C", i32), ("f", i32), ("act", i32)]
    KIND, FN = OP_CBN_APPLY, "gode_cbn_apply"


class CbnBwdOp(_Op):
    _fields_ = [("g_a", ptr), ("a", ptr), ("src", ptr), ("bias", ptr), ("mean", ptr), ("invstd", ptr), ("gb", ptr),
                ("gadd", ptr), ("work", ptr), ("dgb", ptr), ("dbias", ptr), ("g_out", ptr), ("ss", i64 * 4), ("gos", i64 * 4),
                ("N", i32), ("H", i32), ("W", i32), ("C", i32), ("f", i32), ("act", i32), ("eval_mode", i32), ("pad_", i32)]
    KIND, FN = OP_CBN_BWD, "gode_cbn_bwd"


class GresOutOp(_Op):
    _fields_ = [("main", ptr), ("sc", ptr), ("b_main", ptr), ("b_sc", ptr), ("y", ptr), ("N", i32), ("H", i32), ("W", i32),
                ("C", i32), ("f", i32), ("down", i32)]
    KIND, FN = OP_GRES_OUT, "gode_gres_out"


class GresOutBwdOp(_Op):
    _fields_ = [("g_y", ptr), ("g_sc", ptr), ("g_main", ptr), ("db", ptr), ("work", ptr), ("gys", i64 * 4), ("N", i32),
                ("H", i32), ("W", i32), ("C", i32), ("f", i32), ("down", i32)]
    KIND, FN = OP_GRES_OUT_BWD, "gode_gres_out_bwd"


class SnOp(_Op):
    _fields_ = [("wbar", ptr), ("u", ptr), ("v", ptr), ("wout", ptr), ("sigma", ptr), ("work", ptr), ("h", i32), ("w", i32)]
    KIND, FN = OP_SN_FWD, "gode_sn_fwd"


class SnBwdOp(_Op):
    _fields_ = [("G", ptr), ("wbar", ptr), ("u", ptr), ("v", ptr), ("sigma", ptr), ("dwbar", ptr), ("work", ptr), ("h", i32),
                ("w", i32)]
    KIND, FN = OP_SN_BWD, "gode_sn_bwd"


class FcActOp(_Op):
    _fields_ = [("y", ptr), ("b", ptr), ("out", ptr), ("M", i64), ("C", i32), ("act", i32), ("key", i64), ("layer", i32),
                ("p", f32)]
    KIND, FN = OP_FC_ACT, "gode_fc_act"


class FcActBwdOp(_Op):
    _fields_ = [("g_out", ptr), ("out", ptr), ("g_y", ptr), ("db", ptr), ("work", ptr), ("M", i64), ("C", i32), ("act", i32),
                ("key", i64), ("layer", i32), ("p", f32), ("accumulate", i32), ("pad_", i32)]
    KIND, FN = OP_FC_ACT_BWD, "gode_fc_act_bwd"


class BceProbOp(_Op):
    _fields_ = [("p", ptr), ("t", ptr), ("grad", ptr), ("loss", ptr), ("n", i64), ("gscale", f32), ("accumulate", i32)]
    KIND, FN = OP_BCE_PROB, "gode_bce_prob"


class BceTOp(_Op):
    _fields_ = [("logits", ptr), ("target", ptr), ("grad", ptr), ("loss", ptr), ("n", i64), ("gscale", f32), ("accumulate", i32)]
    KIND, FN = OP_BCE_T, "gode_bce_logits_t"


class ResizeU8Op(_Op):
    _fields_ = [("src", ptr), ("dst", ptr), ("dst_f32", ptr), ("y_first", ptr), ("y_count", ptr), ("y_w", ptr), ("x_first", ptr),
                ("x_count", ptr), ("x_w", ptr), ("ss", i64 * 4), ("F", i32), ("Hin", i32), ("Win", i32), ("C", i32), ("out_h", i32),
                ("out_w", i32), ("ky", i32), ("kx", i32)]
    KIND, FN = OP_RESIZE_U8, "gode_resize_u8"


class ClipGatherOp(_Op):
    _fields_ = [("frames", ptr), ("first", ptr), ("out", ptr), ("n_frames", i64), ("frame_elems", i64), ("B", i32), ("T", i32),
                ("sub", f32), ("inv", f32)]
    KIND, FN = OP_CLIP_GATHER, "gode_clip_gather"


class RotClipsOp(_Op):
    _fields_ = [("images", ptr), ("cs", ptr), ("out", ptr), ("raw", ptr), ("n", i32), ("K", i32), ("H", i32), ("W", i32),
                ("in_u8", i32), ("in_scale", f32), ("in_shift", f32), ("cval", f32)]
    KIND, FN = OP_ROT_CLIPS, "gode_rot_clips"


class VideoGridOp(_Op):
    _fields_ = [("src", ptr), ("xs", i64 * 5), ("rgb", ptr), ("idx", ptr), ("B", i32), ("C", i32), ("T", i32), ("H", i32),
                ("W", i32), ("rows", i32), ("cols", i32), ("mode", i32)]
    KIND, FN = OP_VIDEO_GRID, "gode_video_grid"


class LatentDrawOp(_Op):
    _fields_ = [("x", ptr), ("content", ptr), ("sel_t", ptr), ("cls", ptr), ("call_dev", ptr), ("seed", i64), ("traj0", i64),
                ("n", i32), ("outer", i32), ("inner", i32), ("T", i32), ("n_all", i32), ("C", i32), ("stream", i32),
                ("call", i32)]
    KIND, FN = OP_LATENT_DRAW, "gode_latent_draw"


class DiffAugOp(_Op):
    _fields_ = [("x", ptr), ("out", ptr), ("work", ptr), ("call_dev", ptr), ("xs", i64 * 5), ("seed", i64), ("g0", i64),
                ("N", i32), ("C", i32), ("D", i32), ("H", i32), ("W", i32), ("mask", i32), ("backward", i32), ("stream", i32),
                ("call", i32), ("pad_", i32)]
    KIND, FN = OP_DIFFAUG, "gode_diffaug"


class AdamNoiseTensor(C.Structure):
    _fields_ = [("p", ptr), ("g", ptr), ("m", ptr), ("v", ptr), ("n", i64), ("noise_off", i64)]


class AdamOp(_Op):
    _fields_ = [("p", ptr), ("g", ptr), ("m", ptr), ("v", ptr), ("n", i64), ("lr", f32), ("beta1", f32),
                ("beta2", f32), ("eps", f32), ("weight_decay", f32), ("gscale", f32), ("step", i32), ("pad_", i32)]
    KIND, FN = OP_ADAM, "gode_adam_l2"


class PackOp(C.Structure):
    """Not an _Op: it has no (op*, stream) entry point; gode_run batches runs of it, run_one calls gode_pack_weights."""
    _fields_ = [("g", ConvGeom), ("dir", i32), ("co_canon", i32), ("w", ptr), ("wpack", ptr), ("co_perm", ptr)]
    KIND = OP_PACK


_OPS = _Op.__subclasses__()
_STRUCTS = {0: ConvGeom, REC_ADAM_NOISE: AdamNoiseTensor, OP_PACK: PackOp, **{st.KIND: st for st in _OPS}}

# every entry point that is not an op's FN: name -> (argtypes, restype)
_PROTOS = {
    "gode_igemm_stats_rows": ([ptr], cint),
    "gode_igemm_stats_rows0": ([ptr], cint),
    "gode_igemm_stats_segments": ([ptr, i32, ptr], cint),
    "gode_igemm_model_cycles": ([ptr], C.c_double),
    "gode_igemm_family": ([ptr], cint),
    "gode_igemm_dead_taps": ([ptr], C.c_double),
    "gode_igemm_launch_info": ([ptr, ptr], cint),
    "gode_igemm_launch_cell": ([ptr, ptr], cint),
    "gode_igemm_work_size": ([ptr], i64),
    "gode_col2im_launch_kind": ([ptr, ptr], cint),
    "gode_video_grid_launch_kind": ([ptr, ptr], cint),
    "gode_gif_lzw_bound": ([i64], i64),
    "gode_gif_lzw": ([ptr, i64, i32, ptr, i64], i64),
    "gode_pack_size": ([ptr, cint], i64),
    "gode_pack_weights": ([ptr, cint, ptr, ptr, ptr, i32, ptr], cint),
    "gode_wgrad_work_size": ([ptr], i64),
    "gode_wgrad_auto_splits": ([ptr], cint),
    "gode_bn_bwd_work_size": ([i64, i32], i64),
    "gode_ode_bwd_work_size": ([i32], i64),
    "gode_ode_bwd_steps_size": ([i32, i32, i32, i32], i64),
    "gode_odernn_bwd_work_size": ([i32], i64),
    "gode_odernn_sync_size": ([i32], i64),
    "gode_sde_bwd_work_size": ([i32], i64),
    "gode_cde_sync_size": ([i32], i64),
    "gode_cde_state_size": ([i32, i32], i64),
    "gode_cde_bwd_work_size": ([i32], i64),
    "gode_gru_bwd_work_size": ([i32], i64),
    "gode_ode_fwd_multi": ([ptr, i32, ptr], cint),
    "gode_ode_bwd_multi": ([ptr, i32, ptr], cint),
    "gode_odernn_fwd_multi": ([ptr, i32, ptr], cint),
    "gode_odernn_bwd_multi": ([ptr, i32, ptr], cint),
    "gode_odernn_fwd_route": ([ptr, i32, ptr], cint),
    "gode_odernn_bwd_route": ([ptr, i32, ptr], cint),
    "gode_gru_fwd_multi": ([ptr, i32, ptr], cint),
    "gode_gru_bwd_multi": ([ptr, i32, ptr], cint),
    "gode_chstats_rows": ([i64], cint),
    "gode_cbn_bwd_work_size": ([i32, i32, i32, i32], i64),
    "gode_gres_out_bwd_work_size": ([i32, i32, i32, i32, i32, i32], i64),
    "gode_fc_act_bwd_work_size": ([i64, i32], i64),
    "gode_dropout_mask": ([ptr, i64, u64, u32, f32, ptr], cint),
    "gode_scale": ([ptr, ptr, i64, f32, cint, ptr], cint),
    "gode_adam_multi": ([ptr, i32, i64, f32, f32, f32, f32, f32, f32, i32, ptr], cint),
    "gode_adam_multi_dev": ([ptr, i32, i64, f32, f32, f32, f32, f32, ptr, ptr], cint),
    "gode_adam_noise_multi": ([ptr, i32, i64, f32, f32, f32, f32, f32, f32, i32, u64, u32, u32, f32, ptr], cint),
    "gode_adam_noise_multi_dev": ([ptr, i32, i64, f32, f32, f32, f32, f32, ptr, u64, u32, f32, ptr], cint),
    "gode_param_noise": ([ptr, i64, u64, u32, u32, i64, f32, i32, ptr], cint),
    "gode_dnoise_normals": ([ptr, i64, u64, u32, u32, u32, i64, i32, ptr], cint),
    "gode_diffaug_chunks": ([i32, i32, i32], i32),
    "gode_diffaug_work_size": ([i32, i32, i32, i32, i32], i64),
    "gode_diffaug_params": ([ptr, ptr, i64, u64, u32, u32, i64, i32, i32], cint),
    "gode_ode_step_chunks": ([ptr, i64], i64),
    "gode_ode_step": ([ptr, i32, i64, i32, f32, f32, f32, f32, f32, ptr, ptr], cint),
    "gode_axpy_multi": ([ptr, i32, i64, f32, ptr, ptr, f32, ptr, ptr, ptr], cint),
    "gode_run": ([ptr, ptr, i32, ptr], cint),
    "gode_lanes_create": ([ptr], cint),
    "gode_lanes_destroy": ([ptr], cint),
    "gode_lanes_stream": ([ptr], ptr),
    "gode_run_lanes": ([ptr, ptr, ptr, i32, i32, i32, i32, ptr], cint),
    "gode_run_pair": ([ptr, ptr, ptr, ptr, i32, i32, i32, ptr], cint),
    "gode_version": (None, cint),
    "gode_sizeof": ([cint], cint),
}

EXPORTS = [st.FN for st in _OPS] + list(_PROTOS)

_lib = None


def lib():
    """The loaded library; raises RuntimeError (never falls back) when it is missing or inconsistent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                           "(hipcc --offload-arch=gfx950); there is no CPU or PyTorch fallback")
    L = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(L, name):
            raise RuntimeError(f"libgode.so does not export {name}")
        fn = getattr(L, name)
        fn.argtypes, fn.restype = _PROTOS.get(name, ([ptr, ptr], cint))     # an op's FN: (const op*, hipStream_t)
    for kind, st in _STRUCTS.items():
        if L.gode_sizeof(kind) != C.sizeof(st):
            raise RuntimeError(f"ABI mismatch for op kind {kind}: C {L.gode_sizeof(kind)} != ctypes {C.sizeof(st)}")
    _lib = L
    return L


def check(rc, what="gode call"):
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}" + (" (hipError)" if rc > 0 else " (argument/shape error)"))


# Measurement hook (bench.py's iteration roofline / per-class time split): when TRACE is a list, every op is launched
# on its own between two stream events and (op, start_event, end_event) is appended.  None (default): no overhead
# beyond one comparison per program.
TRACE = None


def _traced(op, stream, launch):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    TRACE.append((op, e0, e1))


# Process-wide count of launches through the three funnels below (Program.run, run_one, call).  A plan that ran its last
# call through LanesProgram compares the count with the one it saw then: equal means that nothing of libgode -- an
# optimiser step, another plan, a trainer -- has been queued in between.
LAUNCHES = 0


def call(tag, launch):
    """Entry points that take no op struct (gode_adam_multi, gode_scale): `tag` stands in for the op in TRACE."""
    global LAUNCHES
    LAUNCHES += 1
    if TRACE is not None:
        return _traced(tag, None, launch)
    launch()


class Program:
    """A fixed list of op structs executed by one gode_run call.  The structs stay alive (and patchable) here."""

    def __init__(self, ops):
        self.ops = list(ops)
        n = len(self.ops)
        self.kinds = (i32 * n)(*[op.KIND for op in self.ops])
        self.ptrs = (ptr * n)(*[C.addressof(op) for op in self.ops])
        self.n = n

    def run(self, stream):
        global LAUNCHES
        LAUNCHES += 1
        if TRACE is not None:
            for op in self.ops:
                run_one(op, stream)
            return
        check(lib().gode_run(self.kinds, self.ptrs, self.n, stream), "gode_run")


LANES_ORDERED, LANES_OVERLAP = 0, 1


class Lanes:
    """A gode_lanes object (include/gode.h): the side stream of the two-lane runner and its events, library-owned."""

    # An object whose owner is gone goes back here (per device) and serves the next owner; none is destroyed before the
    # process ends.  torch keeps the side stream's handle past the owner's life -- the pinned staging buffers remember the
    # streams they were copied on and record an event on each when they are freed -- so a destroyed stream would be used.
    _free = {}

    def __init__(self, device_index):
        """Call with `device_index` current (the stream is created on the current device)."""
        self.device_index = device_index
        pool = Lanes._free.setdefault(device_index, [])
        if pool:
            self.handle = pool.pop()
        else:
            self.handle = ptr()
            check(lib().gode_lanes_create(C.byref(self.handle)), "gode_lanes_create")
        self.stream_ptr = lib().gode_lanes_stream(self.handle)

    _shared = {}

    @classmethod
    def shared(cls, device_index, second):
        """The device's two lanes objects, shared by every plan: one for first plans, one for the SECOND plan of a pair
        (gode_run_pair).  Streams are few -- the runtime spreads them over a handful of hardware queues, and one more stream
        in a process cost its generator step 2-5 % -- and sharing is safe: a call overlaps only when no
        libgode launch was issued since the same plan's previous call, so two plans never interleave on an object without an
        ordered call in between, which waits for everything queued and for no state the object carries.  Call with
        `device_index` current."""
        key = (device_index, bool(second))
        if key not in cls._shared:
            cls._shared[key] = cls(device_index)
        return cls._shared[key]

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h and not sys.is_finalizing():
            Lanes._free.setdefault(self.device_index, []).append(h)


class LanesProgram(Program):
    """A program whose ops [0, n_front) run on a Lanes object's side stream (gode_run_lanes); release_after: the last op
    of the main lane that touches a buffer the front writes."""

    def __init__(self, ops, n_front, release_after):
        super().__init__(ops)
        self.n_front, self.release_after = int(n_front), int(release_after)

    def run_lanes(self, lanes, mode, stream):
        global LAUNCHES
        LAUNCHES += 1
        check(lib().gode_run_lanes(lanes.handle, self.kinds, self.ptrs, self.n, self.n_front, self.release_after, mode,
                                   stream), "gode_run_lanes")


class PairProgram(Program):
    """A program that runs on a Lanes object's own stream but for its last n_tail ops (gode_run_pair): the next call's
    program, on the peer object, runs next to it."""

    def __init__(self, ops, n_tail=1):
        super().__init__(ops)
        self.n_tail = int(n_tail)

    def run_pair(self, lanes, peer, mode, stream):
        global LAUNCHES
        LAUNCHES += 1
        check(lib().gode_run_pair(lanes.handle, None if peer is None else peer.handle, self.kinds, self.ptrs, self.n,
                                  self.n_tail, mode, stream), "gode_run_pair")


def run_one(op, stream):
    global LAUNCHES
    LAUNCHES += 1
    if op.KIND == OP_PACK:
        launch = lambda: check(lib().gode_pack_weights(C.byref(op.g), op.dir, op.w, op.wpack, op.co_perm, op.co_canon,  # noqa: E731
                                                       stream), "gode_pack_weights")
        return _traced(op, stream, launch) if TRACE is not None else launch()
    if TRACE is not None:
        return _traced(op, stream, lambda: _run_one(op, stream))
    _run_one(op, stream)


def _run_one(op, stream):
    check(getattr(lib(), op.FN)(C.byref(op), stream), op.FN)
