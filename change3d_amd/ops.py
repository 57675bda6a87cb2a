"""Thin torch-tensor wrappers over the C ABI (include/change3d_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every
computation below is a hand-written gfx950 kernel in libchange3d_hip.so.  All functions
launch on `torch.cuda.current_stream()` and never synchronise.
"""
import ctypes as C
import math
import os

import torch

from . import _lib as L
from ._lib import (OPT_CONVT_MFMA, OPT_DW_FWD_HV, OPT_DW_RING, OPT_DW_T4, OPT_FOLD_SE, OPT_FUSE_WGRAD, OPT_MASK_IN_DGRAD, OPT_PW_CDG, OPT_PW_CFWD, OPT_PW_WGRAD_V2, OPT_SIDE_STREAM, OPT_STEM_MFMA, STAGE_NO_WEIGHT_IMAGES, STAGE_SEPARATE_FINALIZE,  # noqa: F401
                   STAGE_SEPARATE_RESIDUAL, STAGE_SEPARATE_WGRAD)
from ._lib import (DT_BF16, DT_F32, EPI_ADD, EPI_STATS, EPI_STORE, EPI_SWISH_SE_BWD, PRO_AFFINE2,  # noqa: F401
                   PRO_BN_SE_SWISH, PRO_NONE, ROWS_DENSE, ROWS_FRAME, ROWS_S2SHIFT, ROWS_STRIDE2, SC_BN,
                   SC_IDENTITY, SC_NONE, SC_RAW, STAT_STRIPES)


def cpad(c):
    return (c + 7) // 8 * 8


def dt_code(dtype):
    if dtype == torch.float32:
        return DT_F32
    if dtype == torch.bfloat16:
        return DT_BF16
    raise TypeError(f"unsupported activation dtype {dtype} (float32 | bfloat16)")


TRACE = None      # debug: list of (kernel name, [(shape, dtype, checksum), ...]) when tracing is on
_TRACE_ARGS = []


def trace_begin():
    """Debug aid (tools/determinism.py): after every launch, checksum every tensor the wrapper
    passed to it.  Two runs from identical state must give identical traces; the first differing
    entry names the kernel whose output is not reproducible."""
    global TRACE
    TRACE = []
    _TRACE_ARGS.clear()


def trace_end():
    global TRACE
    t, TRACE = TRACE, None
    _TRACE_ARGS.clear()
    return t


def _p(t):
    if t is None:
        return None
    if TRACE is not None:
        _TRACE_ARGS.append(t)
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def require_gpu(t, what="input"):
    if not t.is_cuda:
        raise L.Change3DHipError(
            f"{what} is on {t.device}: the Change3D hot path runs only as HIP kernels on an MI355X "
            f"(no CPU fallback). Use the oracle in oracle/ for CPU reference results.")


PROFILE = None  # dict: kernel name -> list of (start_event, end_event, algorithmic_bytes) when enabled


def profile_begin(serial=True, detail=False):
    """Per-kernel HIP-event profile of everything launched until `profile_end()`: the wrappers below time their own
    launches, the C++ stage driver times the launches it enqueues itself (`c3d_prof_begin`).  serial: weight
    gradients run inline on the launch stream, so an event pair brackets exactly one kernel."""
    global PROFILE, PROFILE_DETAIL, _prof_side_was, SIDE_STREAM
    PROFILE = {}
    PROFILE_DETAIL = detail
    _prof_side_was = SIDE_STREAM
    if serial:
        SIDE_STREAM = False
    L.check(L.lib().c3d_prof_begin((1 if serial else 0) | (2 if detail else 0)), "c3d_prof_begin")


def profile_end():
    """Returns {name: dict(launches, ms_total, bytes_total)} and disables profiling."""
    global PROFILE, PROFILE_DETAIL, SIDE_STREAM
    prof, PROFILE = PROFILE, None
    PROFILE_DETAIL = False
    SIDE_STREAM = _prof_side_was
    rows = (L.ProfRow * 512)()
    n = C.c_int32(0)
    L.check(L.lib().c3d_prof_end(rows, 512, C.byref(n)), "c3d_prof_end")   # synchronises the device
    out = {}
    for name, recs in (prof or {}).items():
        ms = sum(e0.elapsed_time(e1) for e0, e1, _ in recs)
        out[name] = dict(launches=len(recs), ms_total=ms, bytes_total=float(sum(b for _, _, b in recs)))
    for r in rows[:n.value]:
        d = out.setdefault(r.name.decode(), dict(launches=0, ms_total=0.0, bytes_total=0.0))
        d["launches"] += r.launches
        d["ms_total"] += r.ms_total
        d["bytes_total"] += r.bytes_total
    return out


_prof_side_was = True
PROFILE_DETAIL = False  # profile keys carry the GEMM shape/mode (bench.py --kernel-table)


# ---------------------------------------------------------------------------- weights version
# Bumped by everything in this package that writes parameters or BatchNorm buffers IN PLACE without going through
# nn.Module hooks (FusedAdam.launch, broadcast_module_state, ParamArena placement): X3DResStage compares it with the
# version its folded-BatchNorm weights were built from, so an eval forward never runs on stale folded weights.
_weights_version = [0]


def weights_version():
    return _weights_version[0]


def bump_weights_version():
    _weights_version[0] += 1


# ---------------------------------------------------------------------------- side stream
# Weight gradients (and the stem's input gradient) are leaves of the backward graph.  Launched on a
# side stream they fill the chip while the data-gradient chain sits in single-workgroup coefficient
# kernels and in kernel tails (eager launch only: a HIP-graph replay runs its branches one after
# another).  Everything is joined back at the end of the autograd pass (engine callback), so callers
# see ordinary stream semantics: after backward() returns, p.grad is safe to read on the current stream.
SIDE_STREAM = os.environ.get("C3D_WGRAD_SIDE", "1") != "0"
_side_streams = {}
_side_pending = []      # (seq, done_event, tensors kept alive until the event has been waited for)
_side_state = {"seq": 0}


def set_option(option, value):
    """Run-time options of the library (include/change3d_hip.h: C3D_OPT_*)."""
    L.check(L.lib().c3d_set_option(int(option), int(value)), "c3d_set_option")


def last_kernel():
    """Name, with template arguments, of the kernel this thread launched last through the library's large-LDS launcher
    (c3d_last_kernel): how a test knows which kernel a dispatcher picked."""
    return L.lib().c3d_last_kernel().decode()


def launch_count():
    """Kernels this thread has launched through that launcher so far (c3d_launch_count): the difference around a call is 2
    where c3d_pw_gemm answered it with a separate c3d_bn_se_finalize launch in front of the GEMM."""
    return int(L.lib().c3d_launch_count())


def side_run(fn, *tensors):
    """Run `fn` (kernel launches) on the side stream after everything issued so far on the current
    stream.  Only inside an autograd backward pass (that is where the join callback can be queued: one
    per call, joining is idempotent); anywhere else `fn` runs inline."""
    in_backward = False
    if SIDE_STREAM:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(side_join)
            in_backward = True
        except RuntimeError:
            pass
    if not in_backward:
        fn()
        return
    dev = torch.cuda.current_device()
    st = _side_streams.get(dev)
    if st is None:
        st = _side_streams[dev] = torch.cuda.Stream(dev)
    ev = torch.cuda.Event()
    ev.record()
    with torch.cuda.stream(st):
        st.wait_event(ev)
        fn()
        done = torch.cuda.Event()
        done.record()
    _side_state["seq"] += 1
    _side_pending.append((_side_state["seq"], done, [t for t in tensors if t is not None]))


def side_mark():
    return _side_state["seq"]


def side_join(upto=None):
    """Make the current stream wait for the side work issued up to mark `upto` (default: all of it --
    including the C++ stage driver's own side stream) and release the tensors it was reading."""
    last = None
    while _side_pending and (upto is None or _side_pending[0][0] <= upto):
        last = _side_pending.pop(0)
    if last is not None:
        torch.cuda.current_stream().wait_event(last[1])
    if upto is None and _driver_keep:
        rc = L.lib().c3d_side_join(_stream())
        if rc != 0:
            raise L.Change3DHipError(f"c3d_side_join failed with code {rc}")
        _driver_keep.clear()


_driver_keep = []   # workspaces the stage driver's side stream may still be reading (freed at the next full join)


def keep_until_join(*tensors):
    """Keep `tensors` alive until the next full `side_join()`; inside an autograd backward pass that join is
    queued as an end-of-pass callback, so after backward() returns p.grad is safe to read."""
    _driver_keep.extend(t for t in tensors if t is not None)
    try:
        torch.autograd.Variable._execution_engine.queue_callback(side_join)
    except RuntimeError:   # not inside backward(): join now
        side_join()


def _detail(name, a):
    if PROFILE is None or not PROFILE_DETAIL:
        return name
    if name == "c3d_pw_gemm":
        return f"{name}[M={a.M} K={a.K} N={a.N} pro={a.pro_mode} epi={a.epi_mode} rows={a.row_mode}]"
    return f"{name}[M={a.M} K={a.K} N={a.N} q={a.q_mode} rows={a.row_mode}]"


def _launch(name, nbytes, fn, *args):
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        prof.setdefault(name, []).append((e0, e1, nbytes))
    else:
        rc = fn(*args)
    if rc != 0:
        raise L.Change3DHipError(f"{name} failed with code {rc}")
    if TRACE is not None:
        TRACE.append((name, [(tuple(t.shape), str(t.dtype), float(t.detach().double().abs().sum().item()))
                             for t in _TRACE_ARGS]))
        _TRACE_ARGS.clear()


def _es(dtype):
    return 4 if dtype == DT_F32 else 2


def grad_of(p):
    """Accumulation target for a parameter gradient (kernels do `+=`)."""
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


# ----------------------------------------------------------------------------- pointwise GEMM
def fin_consume(sums, bn, count, ss, mr, batch=0):
    """c3d_bn_fin for the consumer-side finalisation (c3d_dw333_fwd_fin / c3d_block_out_fwd_fin): `sums` are the
    completed f64 [16][2][C] statistics of an earlier launch; batch > 0: the per-sample layout [batch][Cp][2] of
    c3d_dw333_fwd (BatchNorm_b of a block without SqueezeExcitation, consumed by c3d_pw_gemm's BN_SE_SWISH prologue)."""
    f = L.BnFin()
    f.batch = int(batch)
    f.sums = _p(sums)
    f.gamma, f.beta = _p(bn.weight), _p(bn.bias)
    f.running_mean, f.running_var, f.nbt = _p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked)
    f.ss, f.mr, f.count = _p(ss), _p(mr), float(count)
    f.momentum, f.eps, f.training = float(bn.momentum), float(bn.eps), 1
    return f


WG_NONE, WG_SWISH, WG_ROWS, WG_MASKSUM = 0, 1, 2, 3


def pw_gemm(x, w, y, *, M, K, N, w_sn, w_sk, dtype, x2=None, pro_mode=PRO_NONE, pro_p=None,
            pro_gate=None, epi_mode=EPI_STORE, e1=None, epi_p=None, epi_gate=None, epi_q=None, stats=None,
            rows_per_sample=0, row_mode=ROWS_DENSE, rpg=0, gstride=0, H=0, W=0, res_mode=0,
            x_ptr=None, e1_ptr=None, fin=None, bias=None, pro_out=None, w_img=None, wg_mode=WG_NONE, wg_x3=None, wg_dw=None, wg_mask_out=0,
            add_c=None, add_mr=None, add_sums=None):
    a = L.PwArgs()
    a.w_img = _p(w_img)
    if wg_mode == WG_MASKSUM:   # no weight gradient: the previous block's c3d_block_out_bwd in this epilogue (c3d_pw_args.add_sums)
        a.wg_mode, a.wg_x3 = wg_mode, _p(wg_x3)
    elif wg_mode != WG_NONE:   # weight gradient fused into this data-gradient launch (include/change3d_hip.h c3d_pw_args.wg_mode)
        a.wg_mode, a.wg_x3, a.wg_dw, a.wg_mask_out = wg_mode, _p(wg_x3), _p(wg_dw), int(wg_mask_out)
        a.wg_ws = _ws(wg_dw.device, L.lib().c3d_pw_gemm_wg_ws_floats(K, N)).data_ptr()
    a.add_c, a.add_mr, a.add_sums = _p(add_c), _p(add_mr), _p(add_sums)
    if fin is not None:
        a.fin = fin
    a.bias = _p(bias)
    a.pro_out = _p(pro_out)
    a.x = x_ptr if x_ptr is not None else _p(x)
    a.x2 = _p(x2)
    a.y = _p(y)
    a.e1 = e1_ptr if e1_ptr is not None else _p(e1)
    a.w = _p(w)
    a.pro_p, a.pro_gate, a.epi_p, a.epi_gate, a.stats = _p(pro_p), _p(pro_gate), _p(epi_p), _p(epi_gate), _p(stats)
    a.epi_q = _p(epi_q)
    a.M, a.gstride, a.rows_per_sample = M, gstride, rows_per_sample
    a.K, a.Kp, a.N, a.Np = K, cpad(K), N, cpad(N)
    a.w_sn, a.w_sk = w_sn, w_sk
    a.row_mode, a.rpg, a.H, a.W = row_mode, rpg, H, W
    a.pro_mode, a.epi_mode, a.res_mode, a.dtype = pro_mode, epi_mode, res_mode, dtype
    _launch(_detail("c3d_pw_gemm", a), a.M * (a.Kp * (2 if x2 is not None else 1) + a.Np * (2 if (e1 is not None or e1_ptr is not None) else 1)) * _es(dtype), L.lib().c3d_pw_gemm, C.byref(a), _stream())


def pw_weight_image_bytes(N, K, dtype):
    """Bytes of the LDS image of an (N, K) pointwise weight for `c3d_pw_args.w_img` (0: shape not taken)."""
    return int(L.lib().c3d_pw_weight_image_bytes(cpad(N), cpad(K), dtype))


def pw_pack_weights(items, dtype):
    """items: (w, img, N, K, w_sn, w_sk) tuples; one launch per 64 images (`c3d_pw_pack_weights`)."""
    descs = (L.PwPackDesc * len(items))()
    for d, (w, img, N, K, sn, sk) in zip(descs, items):
        d.w, d.img, d.N, d.Np, d.K, d.Kp, d.w_sn, d.w_sk = _p(w), _p(img), N, cpad(N), K, cpad(K), sn, sk
    _launch("c3d_pw_pack_weights", 0, L.lib().c3d_pw_pack_weights, descs, len(items), dtype, _stream())


_wgrad_ws = {}


def _ws(device, n_floats):
    key = (device.index, _stream())   # one workspace per stream: weight gradients may run on a side stream
    buf = _wgrad_ws.get(key)
    if buf is None or buf.numel() < n_floats:
        buf = torch.empty(int(n_floats), dtype=torch.float32, device=device)
        _wgrad_ws[key] = buf
    return buf


def pw_wgrad(p, q, dw, *, M, K, N, dw_sn, dw_sk, dtype, p2=None, p_coef=None, q_mode=PRO_NONE, q_ss=None,
             q_gate=None, rows_per_sample=0, row_mode=ROWS_DENSE, rpg=0, gstride=0, H=0, W=0, dy=0, dx=0,
             q_ptr=None, dw_ptr=None, taps=0, dw_tap_stride=0, chain_ws=None, p_fin=None):
    """chain_ws: a caller-owned workspace tensor (c3d_pw_wgrad_ws_floats(N, K) floats) -> a CHAINED launch (c3d_pw_wgrad_args.chain):
    its partials stay pending in chain_ws until the next chained launch or pw_wgrad_flush(); alternate two workspaces.
    p_fin: a c3d_bn_fin (L.BnFin) whose completed sums give the AFFINE2 coefficients of p (c3d_pw_wgrad_args.p_fin), as pw_gemm's fin."""
    a = L.PwWgradArgs()
    if p_fin is not None:
        a.p_fin = p_fin
    a.p, a.p2 = _p(p), _p(p2)
    a.q = q_ptr if q_ptr is not None else _p(q)
    a.dw = dw_ptr if dw_ptr is not None else _p(dw)
    ws = chain_ws if chain_ws is not None else _ws(p.device, L.lib().c3d_pw_wgrad_ws_floats(N, K))
    a.ws = ws.data_ptr()
    a.chain = 1 if chain_ws is not None else 0
    a.p_coef, a.q_ss, a.q_gate = _p(p_coef), _p(q_ss), _p(q_gate)
    a.M, a.gstride, a.rows_per_sample = M, gstride, rows_per_sample
    a.K, a.Kp, a.N, a.Np = K, cpad(K), N, cpad(N)
    a.dw_sn, a.dw_sk = dw_sn, dw_sk
    a.row_mode, a.rpg, a.H, a.W, a.dy, a.dx = row_mode, rpg, H, W, dy, dx
    a.q_mode, a.dtype = q_mode, dtype
    a.taps, a.dw_tap_stride = taps, dw_tap_stride
    _launch(_detail("c3d_pw_wgrad", a), a.M * (a.Np * (2 if p2 is not None else 1) + a.Kp) * _es(dtype), L.lib().c3d_pw_wgrad, C.byref(a), _stream())


def pw_wgrad_flush():
    """Reduce the pending partials of the last chained pw_wgrad launch (include/change3d_hip.h: c3d_pw_wgrad_flush)."""
    L.check(L.lib().c3d_pw_wgrad_flush(_stream()), "c3d_pw_wgrad_flush")


# ------------------------------------------------------------------------------- BN / SE
def bn_finalize(sums, count, bn, C_, ss, mr, training, stripes=1):
    _launch("c3d_bn_finalize", 0, L.lib().c3d_bn_finalize, _p(sums), stripes, float(count), _p(bn.weight), _p(bn.bias), _p(bn.running_mean),
                                    _p(bn.running_var), _p(bn.num_batches_tracked) if training else None,
                                    float(bn.momentum), float(bn.eps), C_, cpad(C_), 1 if training else 0,
                                    _p(ss), _p(mr), _stream())


def bn_se_finalize(nc, B, cnt, bn, se, C_, ss, mr, gate, hid, training):
    if se is not None:
        w1, b1, w2, b2 = se.block[0].weight, se.block[0].bias, se.block[2].weight, se.block[2].bias
        Cr = w1.shape[0]
    else:
        w1 = b1 = w2 = b2 = None
        Cr = 0
    _launch("c3d_bn_se_finalize", 0, L.lib().c3d_bn_se_finalize, _p(nc), B, float(cnt), _p(bn.weight), _p(bn.bias), _p(bn.running_mean),
                                       _p(bn.running_var), _p(bn.num_batches_tracked) if training else None,
                                       float(bn.momentum), float(bn.eps), C_, cpad(C_), 1 if training else 0,
                                       _p(w1), _p(b1), _p(w2), _p(b2), Cr, _p(ss), _p(mr), _p(gate), _p(hid),
                                       _stream())


def bn_bwd_coef(dsums, count, bn, mr, C_, coef, stripes=1):
    _launch("c3d_bn_bwd_coef", 0, L.lib().c3d_bn_bwd_coef, _p(dsums), stripes, float(count), _p(bn.weight), _p(mr), C_, cpad(C_), _p(coef),
                                    _p(grad_of(bn.weight)), _p(grad_of(bn.bias)), _stream())


def se_bn_bwd_coef(nc3, ncf, B, cnt, bn, mr, ss, se, gate, hid, C_, coefA, coefC, coefB):
    if se is not None:
        c1, c2 = se.block[0], se.block[2]
        args = (_p(c1.weight), _p(c2.weight), _p(gate), _p(hid), c1.weight.shape[0])
        gargs = (_p(grad_of(c1.weight)), _p(grad_of(c1.bias)), _p(grad_of(c2.weight)), _p(grad_of(c2.bias)))
    else:
        args = (None, None, None, None, 0)
        gargs = (None, None, None, None)
    _launch("c3d_se_bn_bwd_coef", 0, L.lib().c3d_se_bn_bwd_coef, _p(nc3), _p(ncf), B, float(cnt), _p(bn.weight), _p(mr), _p(ss), C_, cpad(C_),
                                       *args, _p(coefA), _p(coefC), _p(coefB), _p(grad_of(bn.weight)),
                                       _p(grad_of(bn.bias)), *gargs, _stream())


# ------------------------------------------------------------------------------ depthwise
def dw_fwd(x, ss, w, y, nc, B, T, H, W, C_, stride, dtype):
    _launch("c3d_dw333_fwd", (x.numel() + y.numel()) * _es(dtype), L.lib().c3d_dw333_fwd, _p(x), _p(ss), _p(w), _p(y), _p(nc), B, T, H, W, C_, cpad(C_), stride, dtype,
                                  _stream())


def dw_fwd_fin(x, fin, w, y, nc, B, T, H, W, C_, stride, dtype):
    _launch("c3d_dw333_fwd", (x.numel() + y.numel()) * _es(dtype), L.lib().c3d_dw333_fwd_fin, _p(x), C.byref(fin), _p(w), _p(y), _p(nc), B, T, H, W, C_, cpad(C_), stride,
                                  dtype, _stream())


def dw_bwd_fused(t1, b, cA, cB, cC, w, a, ss_a, mr_a, t2, dsums, dw, B, T, H, W, C_, dtype, stride=1):
    """Depthwise backward: data gradient, BatchNorm_a-backward sums and weight gradient in one pass."""
    _launch("c3d_dw333_bwd_fused", (t1.numel() + b.numel() + a.numel() + t2.numel()) * _es(dtype), L.lib().c3d_dw333_bwd_fused,
            _p(t1), _p(b), _p(cA), _p(cB), _p(cC), _p(w), _p(a), _p(ss_a), _p(mr_a), _p(t2), _p(dsums), _p(dw),
            B, T, H, W, C_, cpad(C_), stride, dtype, _stream())


def fin_b_bwd(nc3, batch, bn, count, mr):
    """c3d_bn_fin for c3d_dw333_bwd_fused_fin: BatchNorm_b backward coefficients of a block without SqueezeExcitation from
    the per-sample sums nc3 [batch][Cp][3]; d gamma / d beta accumulate into bn.weight.grad / bn.bias.grad."""
    f = L.BnFin()
    f.sums, f.batch, f.gamma, f.mr, f.count = _p(nc3), int(batch), _p(bn.weight), _p(mr), float(count)
    f.running_mean, f.running_var = _p(grad_of(bn.weight)), _p(grad_of(bn.bias))
    return f


def dw_bwd_fused_fin(t1, b, fin_b, w, a, ss_a, mr_a, t2, dsums, dw, B, T, H, W, C_, dtype, stride=1):
    _launch("c3d_dw333_bwd_fused", (t1.numel() + b.numel() + a.numel() + t2.numel()) * _es(dtype), L.lib().c3d_dw333_bwd_fused_fin,
            _p(t1), _p(b), C.byref(fin_b), _p(w), _p(a), _p(ss_a), _p(mr_a), _p(t2), _p(dsums), _p(dw),
            B, T, H, W, C_, cpad(C_), stride, dtype, _stream())


# ----------------------------------------------------------------------------- elementwise
def block_out_fwd(c, ss_c, shortcut, ss_1, mode, y, M, Cp, dtype):
    _launch("c3d_block_out_fwd", M * Cp * (3 if shortcut is not None else 2) * _es(dtype), L.lib().c3d_block_out_fwd, _p(c), _p(ss_c), _p(shortcut), _p(ss_1), mode, _p(y), M, Cp, dtype,
                                      _stream())


def block_out_fwd_fin(c, fin_c, shortcut, fin_1, mode, y, M, C_, dtype):
    _launch("c3d_block_out_fwd", M * cpad(C_) * (3 if shortcut is not None else 2) * _es(dtype), L.lib().c3d_block_out_fwd_fin, _p(c), C.byref(fin_c), _p(shortcut),
                                      C.byref(fin_1) if fin_1 is not None else None, mode, _p(y), M, C_, cpad(C_), dtype, _stream())


def block_out_bwd(dy, y, c, s_bn, g, mr_c, mr_1, dsums_c, dsums_1, M, C_, dtype):
    _launch("c3d_block_out_bwd", M * cpad(C_) * (5 if s_bn is not None else 4) * _es(dtype), L.lib().c3d_block_out_bwd, _p(dy), _p(y), _p(c), _p(s_bn), _p(g), _p(mr_c), _p(mr_1), _p(dsums_c), _p(dsums_1), M, C_,
                                      cpad(C_), dtype, _stream())


def block_out_bwd_fin(dy, y, c, s_bn, g, mr_c, mr_1, dsums_c, dsums_1, M, C_, dtype, fin_c, fin_1):
    _launch("c3d_block_out_bwd", M * cpad(C_) * (5 if s_bn is not None else 4) * _es(dtype), L.lib().c3d_block_out_bwd_fin, _p(dy), _p(y), _p(c), _p(s_bn), _p(g), _p(mr_c), _p(mr_1), _p(dsums_c), _p(dsums_1), M, C_,
            cpad(C_), dtype, C.byref(fin_c), C.byref(fin_1) if fin_1 is not None else None, _stream())


def frame_absdiff(y, d, B, T, HW, Cp, t_pre, t_post, dtype):
    _launch("c3d_frame_absdiff", B * HW * Cp * 3 * _es(dtype), L.lib().c3d_frame_absdiff, _p(y), _p(d), B, T, HW, Cp, t_pre, t_post, dtype, _stream())


def enhance_apply(y, e, out, B, T, HW, Cp, t_mid, dtype):
    _launch("c3d_enhance_apply", B * HW * Cp * (2 * T + 1) * _es(dtype), L.lib().c3d_enhance_apply, _p(y), _p(e), _p(out), B, T, HW, Cp, t_mid, dtype, _stream())


def enhance_bwd_mask(dout, e, de, B, T, HW, Cp, t_mid, dtype):
    _launch("c3d_enhance_bwd_mask", B * HW * Cp * 3 * _es(dtype), L.lib().c3d_enhance_bwd_mask, _p(dout), _p(e), _p(de), B, T, HW, Cp, t_mid, dtype, _stream())


def enhance_bwd_apply(dout, y, dd, dy, B, T, HW, Cp, t_pre, t_post, dtype):
    _launch("c3d_enhance_bwd_apply", B * HW * Cp * (2 * T + 3) * _es(dtype), L.lib().c3d_enhance_bwd_apply, _p(dout), _p(y), _p(dd), _p(dy), B, T, HW, Cp, t_pre, t_post, dtype,
                                          _stream())


# C3D_STEM_ENHANCE=0: level 0 of the encoder runs block_out_fwd + _EnhanceFn (a stored y and dy) instead of the
# stem_enhance_* kernels below (model/trainer.py::_ClipStemEnhanceFn); same results either way
STEM_ENHANCE = os.environ.get("C3D_STEM_ENHANCE", "1") != "0"


def stem_enhance_fwd(u, ss, out, d, B, T, HW, Cp, t_pre, t_post, t_mid, dtype):
    """out[:, t] = relu(bn(u))[:, t] for t != t_mid and d = |y[:, t_pre] - y[:, t_post]| (billed: T-1 frames read,
    T-1 frames + d written)."""
    _launch("c3d_stem_enhance_fwd", B * HW * Cp * (2 * T - 1) * _es(dtype), L.lib().c3d_stem_enhance_fwd, _p(u), _p(ss), _p(out), _p(d),
            B, T, HW, Cp, t_pre, t_post, t_mid, dtype, _stream())


def stem_enhance_mid(u, ss, e, out, B, T, HW, Cp, t_mid, dtype):
    """out[:, t_mid] = relu(bn(u))[:, t_mid] + relu(e)."""
    _launch("c3d_stem_enhance_mid", B * HW * Cp * 3 * _es(dtype), L.lib().c3d_stem_enhance_mid, _p(u), _p(ss), _p(e), _p(out),
            B, T, HW, Cp, t_mid, dtype, _stream())


def stem_enhance_bwd(dout, u, ss, dd, mr, g, dsums, B, T, HW, C_, t_pre, t_post, dtype):
    """g, dsums of block_out_bwd(enhance_bwd_apply(dout, y, dd), y, u) with y recomputed from (u, ss) (billed: dout, u
    read and g written once, dd once; the partner-frame rows of u are read a second time)."""
    _launch("c3d_stem_enhance_bwd", B * HW * cpad(C_) * (3 * T + 1) * _es(dtype), L.lib().c3d_stem_enhance_bwd, _p(dout), _p(u), _p(ss),
            _p(dd), _p(mr), _p(g), _p(dsums), B, T, HW, C_, cpad(C_), t_pre, t_post, dtype, _stream())


def frame_scatter(src, dst, B, T, HW, Cp, t_dst, accumulate, dtype):
    """dst[:, t_dst] (+)= src for channels-last src [B][HW][Cp], dst [B][T][HW][Cp]."""
    _launch("c3d_frame_scatter", B * HW * Cp * (3 if accumulate else 2) * _es(dtype), L.lib().c3d_frame_scatter, _p(src), _p(dst), B, T, HW, Cp,
            t_dst, 1 if accumulate else 0, dtype, _stream())


# ------------------------------------------------------------------------------------ stem
def stem_fwd(x, w_t, w_xy, u, sums, B, T, H, W, dtype):
    _launch("c3d_stem_fwd", x.numel() * 4 + u.numel() * _es(dtype), L.lib().c3d_stem_fwd, _p(x), _p(w_t), _p(w_xy), _p(u), _p(sums), B, T, H, W, dtype, _stream())


def stem_bwd_dv(x, w_t, w_xy, g0, u, coef, dv, dw_xy, B, T, H, W, dtype):
    _launch("c3d_stem_bwd_dv", x.numel() * 4 + 3 * u.numel() * _es(dtype), L.lib().c3d_stem_bwd_dv, _p(x), _p(w_t), _p(w_xy), _p(g0), _p(u), _p(coef), _p(dv), _p(dw_xy), B, T, H,
                                    W, dtype, _stream())


def stem_bwd_wx(x, w_t, dv, dw_t, dP, B, T, H, W, t_first, n_frames, per_sample, dtype):
    _launch("c3d_stem_bwd_wx", x.numel() * 4 + dv.numel() * _es(dtype), L.lib().c3d_stem_bwd_wx, _p(x), _p(w_t), _p(dv), _p(dw_t), _p(dP), B, T, H, W, t_first, n_frames,
                                    1 if per_sample else 0, dtype, _stream())


# --------------------------------------------------------------------------------- decoder
def convT_fwd(inp, w, bias, skip_ptr, skip_bstride, out, B, h, wd, C_, dtype):
    _launch("c3d_convT4s2_fwd", (inp.numel() + 2 * out.numel()) * _es(dtype), L.lib().c3d_convT4s2_fwd, _p(inp), _p(w), _p(bias), skip_ptr, skip_bstride, _p(out), B, h, wd, C_,
                                     dtype, _stream())


def convT_bwd_data(dout, w, din, B, h, wd, C_, dtype):
    _launch("c3d_convT4s2_bwd_data", (dout.numel() + din.numel()) * _es(dtype), L.lib().c3d_convT4s2_bwd_data, _p(dout), _p(w), _p(din), B, h, wd, C_, dtype, _stream())


CONVT_MFMA = os.environ.get("C3D_CONVT_MFMA", "1") != "0"


def convT_wgrad(t, dout, dw, B, h, wd, C_, dtype):
    """ConvTranspose2d k4s2p1 weight gradient on MFMA (bf16 storage only)."""
    ws = _ws(t.device, L.lib().c3d_convT4s2_wgrad_ws_floats(B, h, wd, C_))
    _launch("c3d_convT4s2_wgrad", (t.numel() + dout.numel()) * _es(dtype), L.lib().c3d_convT4s2_wgrad, _p(t), _p(dout), _p(dw),
            ws.data_ptr(), B, h, wd, C_, dtype, _stream())


def col_sum(x, out, M, C_, dtype):
    _launch("c3d_col_sum", M * cpad(C_) * _es(dtype), L.lib().c3d_col_sum, _p(x), _p(out), M, C_, cpad(C_), dtype, _stream())


def head_fwd(x, w, out, B, H, W, C_, NC, has_sigmoid, dtype):
    _launch("c3d_head3x3_fwd", x.numel() * _es(dtype) + out.numel() * 4, L.lib().c3d_head3x3_fwd, _p(x), _p(w), _p(out), B, H, W, C_, NC, 1 if has_sigmoid else 0, dtype,
                                    _stream())


def head_bwd(dout, prob, x, w, dx, dw, B, H, W, C_, NC, has_sigmoid, dtype):
    ws = _ws(x.device, max(1, L.lib().c3d_head3x3_bwd_ws_floats(B, H, W, NC)))
    _launch("c3d_head3x3_bwd", 2 * x.numel() * _es(dtype) + 2 * dout.numel() * 4, L.lib().c3d_head3x3_bwd, _p(dout), _p(prob), _p(x), _p(w), _p(dx), _p(dw), ws.data_ptr(), B, H, W, C_, NC,
                                    1 if has_sigmoid else 0, dtype, _stream())


# ------------------------------------------------------------------------------ train shell
def bce_dice_fwd(prob, target, sums4, loss):
    _launch("c3d_bce_dice_fwd", prob.numel() * 8, L.lib().c3d_bce_dice_fwd, _p(prob), _p(target), prob.numel(), _p(sums4), _p(loss), _stream())


def bce_dice_bwd(prob, target, sums4, dloss, dprob):
    _launch("c3d_bce_dice_bwd", prob.numel() * 12, L.lib().c3d_bce_dice_bwd, _p(prob), _p(target), _p(sums4), _p(dloss), prob.numel(), _p(dprob),
                                     _stream())


def _nchw_view(x):
    """(B, NC, HW, batch stride, channel stride) of an f32 NCHW view whose pixels are contiguous."""
    B, NC, H, W = x.shape
    assert x.dtype == torch.float32 and (W == 1 or x.stride(3) == 1) and (H == 1 or x.stride(2) == W)
    return B, NC, H * W, x.stride(0), x.stride(1)


def ce2d_fwd(logits, target, ignore_index, sums2, loss):
    B, NC, HW, bs, cs = _nchw_view(logits)
    _launch("c3d_ce2d_fwd", B * HW * (NC * 4 + 8), L.lib().c3d_ce2d_fwd, _p(logits), _p(target), B, NC, HW, bs, cs,
            ignore_index, _p(sums2), _p(loss), _stream())


def ce2d_bwd(logits, target, ignore_index, sums2, dloss, dlogits):
    B, NC, HW, bs, cs = _nchw_view(logits)
    _launch("c3d_ce2d_bwd", B * HW * (NC * 8 + 8), L.lib().c3d_ce2d_bwd, _p(logits), _p(target), _p(sums2), _p(dloss),
            B, NC, HW, bs, cs, ignore_index, _p(dlogits), _stream())


def cossim_fwd(x1, x2, label_change, sums1, loss):
    B, NC, HW, bs1, cs1 = _nchw_view(x1)
    _, _, _, bs2, cs2 = _nchw_view(x2)
    _launch("c3d_cossim_fwd", B * HW * (NC * 8 + 8), L.lib().c3d_cossim_fwd, _p(x1), _p(x2), _p(label_change), B, NC, HW,
            bs1, cs1, bs2, cs2, _p(sums1), _p(loss), _stream())


def cossim_bwd(x1, x2, label_change, dloss, dx1, dx2):
    B, NC, HW, bs1, cs1 = _nchw_view(x1)
    _, _, _, bs2, cs2 = _nchw_view(x2)
    _launch("c3d_cossim_bwd", B * HW * (NC * 16 + 8), L.lib().c3d_cossim_bwd, _p(x1), _p(x2), _p(label_change), _p(dloss),
            B, NC, HW, bs1, cs1, bs2, cs2, _p(dx1), _p(dx2), _stream())


def adam_step(param, grad, exp_avg, exp_avg_sq, n, hp_dev, lr, bc1, bc2_sqrt, beta1, beta2, eps, wd):
    _launch("c3d_adam_step", n * 28, L.lib().c3d_adam_step, _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, _p(hp_dev), lr, bc1, bc2_sqrt,
                                  beta1, beta2, eps, wd, _stream())


def confusion2(prob, target, cm4):
    _launch("c3d_confusion2", prob.numel() * 8, L.lib().c3d_confusion2, _p(prob), _p(target), prob.numel(), _p(cm4), _stream())


def hist2d(a, b, n, hist):
    """hist (uint64-as-int64 [n*n + 1], device) += joint histogram of the int64 label maps a (rows) and b (columns)."""
    _launch("c3d_hist2d", a.numel() * 16, L.lib().c3d_hist2d, _p(a), _p(b), a.numel(), n, _p(hist), _stream())


def bda_confusion(pred_cls, pred_loc, label_loc, label_cls, counts):
    """counts (uint64-as-int64 [4 + n*n + 1], device) += localisation matrix | damage matrix over label_loc > 0 | out-of-range
    labels, of one batch (include/change3d_hip.h: c3d_bda_confusion)."""
    B, n = pred_cls.shape[0], pred_cls.shape[1]
    HW = pred_cls.numel() // (B * n)
    assert pred_cls.is_contiguous() and pred_loc.is_contiguous() and label_loc.is_contiguous() and label_cls.is_contiguous()
    assert pred_cls.dtype == torch.float32 and pred_loc.dtype == torch.float32 and label_loc.dtype == torch.float32
    assert label_cls.dtype == torch.int64 and counts.dtype == torch.int64 and counts.numel() == 4 + n * n + 1
    assert pred_loc.numel() == B * HW and label_loc.numel() == B * HW and label_cls.numel() == B * HW
    _launch("c3d_bda_confusion", B * HW * (n * 4 + 16), L.lib().c3d_bda_confusion, _p(pred_cls), _p(pred_loc), _p(label_loc),
            _p(label_cls), B, n, HW, _p(counts), _stream())


# ------------------------------------------------------------------------------ stage driver
class StageBinding:
    """ctypes descriptor (include/change3d_hip.h: c3d_stage_desc) of one residual stage, bound to the tensors of
    the reference-shaped module tree (`X3DResStage.res_blocks[j].branch2.conv_a.weight`, ...).  Pointers are
    re-read on every call (parameters move when a ParamArena is built or the module is moved; gradients move
    when they are reset): ~600 attribute reads per step, no struct write unless something changed."""

    def __init__(self, stage):
        blocks = list(stage.res_blocks)
        self.n = len(blocks)
        self.blocks = (L.BlockDesc * self.n)()
        self.desc = L.StageDesc()
        self.desc.n_blocks = self.n
        self.desc.blocks = C.cast(self.blocks, C.POINTER(L.BlockDesc))
        self.params, self.buffers = [], []      # (struct, field, grad_struct, grad_field, parameter) / (struct, field, buffer)
        self._grad_refs = None
        for bd, blk in zip(self.blocks, blocks):
            b2 = blk.branch2
            se = b2.norm_b[1] if blk.use_se else None
            bd.cin, bd.cinner, bd.cout, bd.stride = blk.cin, blk.cinner, blk.cout, blk.stride
            bd.se_width = se.block[0].weight.shape[0] if se is not None else 0
            bd.has_sc_conv = 1 if blk.branch1_conv is not None else 0
            bd.has_sc_bn = 1 if blk.branch1_norm is not None else 0
            self.params += [(bd, "w_a", bd, "dw_a", b2.conv_a), (bd, "w_b", bd, "dw_b", b2.conv_b),
                            (bd, "w_c", bd, "dw_c", b2.conv_c)]
            if blk.branch1_conv is not None:
                self.params.append((bd, "w_sc", bd, "dw_sc", blk.branch1_conv))
            bns = [(bd.bn_a, b2.norm_a), (bd.bn_b, b2.norm_b[0]), (bd.bn_c, b2.norm_c)]
            if blk.branch1_norm is not None:
                bns.append((bd.bn_sc, blk.branch1_norm))
            for st, bn in bns:
                self.params += [(st, "gamma", st, "dgamma", (bn, "weight")), (st, "beta", st, "dbeta", (bn, "bias"))]
                self.buffers += [(st, "running_mean", bn, "running_mean"), (st, "running_var", bn, "running_var"),
                                 (st, "num_batches_tracked", bn, "num_batches_tracked")]
            if se is not None:
                self.params += [(bd, "se_w1", bd, "dse_w1", (se.block[0], "weight")), (bd, "se_b1", bd, "dse_b1", (se.block[0], "bias")),
                                (bd, "se_w2", bd, "dse_w2", (se.block[2], "weight")), (bd, "se_b2", bd, "dse_b2", (se.block[2], "bias"))]
        # resolve to the Parameter / buffer OBJECTS once (nn.Module.__getattr__ costs ~1 us per lookup, 600 lookups
        # per stage pass): Parameters keep their identity across .to() / load_state_dict() / arena placement;
        # buffers are REPLACED by Module._apply, which is why X3DResStage._apply drops this binding
        self.params = [(s, f, gs, gf, getattr(*(m if isinstance(m, tuple) else (m, "weight")))) for s, f, gs, gf, m in self.params]
        self.buffers = [(s, f, getattr(mod, attr)) for s, f, mod, attr in self.buffers]
        self._ptr_cache = {}
        self._last = {False: None, True: None}   # pointer signatures of the forward / backward bindings

    def _set(self, st, field, ptr):
        key = (id(st), field)
        if self._ptr_cache.get(key) != ptr:
            setattr(st, field, ptr)
            self._ptr_cache[key] = ptr

    def refresh(self, B, T, H, W, dtype, training, momentum, eps, with_grads):
        d = self.desc
        d.B, d.T, d.H, d.W, d.dtype, d.training = B, T, H, W, dtype, 1 if training else 0
        d.momentum, d.eps = momentum, eps
        # pointer signature of everything bound (data, gradients, buffers): ~0.1 us per tensor; the ctypes structs are
        # rewritten only when it changed (first call, new arena, gradients re-created, module moved)
        if with_grads:
            grads = [p.grad if p.grad is not None else grad_of(p) for _, _, _, _, p in self.params]
            sig = tuple([p.data_ptr() for _, _, _, _, p in self.params] + [g.data_ptr() for g in grads] +
                        [b.data_ptr() for _, _, b in self.buffers])
        else:
            grads = None
            sig = tuple([p.data_ptr() for _, _, _, _, p in self.params] + [b.data_ptr() for _, _, b in self.buffers])
        if sig != self._last[with_grads]:
            for i, (st, f, gs, gf, p) in enumerate(self.params):
                self._set(st, f, p.data_ptr())
                if grads is not None:
                    self._set(gs, gf, grads[i].data_ptr())
            for st, f, b in self.buffers:
                self._set(st, f, b.data_ptr())
            self._last[with_grads] = sig
        self._grad_refs = grads   # keep the bound gradient tensors alive while kernels may write them
        return d

    def sizes(self):
        out = [C.c_int64() for _ in range(4)]
        rc = L.lib().c3d_stage_ws_bytes(C.byref(self.desc), *[C.byref(v) for v in out])
        if rc == -2:   # C3D_E_UNSUPPORTED: the one geometry limit of the stage API (include/change3d_hip.h)
            d = self.desc
            raise L.Change3DHipError(
                f"stage geometry B={d.B} T={d.T} {d.H}x{d.W} is too large: an activation tensor of a stage with <= 224 channels "
                f"must stay under 2 GiB (32-bit offsets in the pointwise kernels); reduce the per-GPU batch "
                f"(bf16 at 256x256, T=3: B <= 96; f32: B <= 48)")
        if rc != 0:
            raise L.Change3DHipError(f"c3d_stage_ws_bytes failed with code {rc}")
        return tuple(int(v.value) for v in out)   # ws_fwd, ws_bwd, y, dx bytes

    def saved(self, blk, name):
        off, n = C.c_int64(), C.c_int64()
        rc = L.lib().c3d_stage_saved(C.byref(self.desc), blk, name.encode(), C.byref(off), C.byref(n))
        return None if rc != 0 else (int(off.value), int(n.value))


def stage_fold_sizes(binding):
    a, b = C.c_int64(), C.c_int64()
    rc = L.lib().c3d_stage_fold_bytes(C.byref(binding.desc), C.byref(a), C.byref(b))
    if rc == -2:   # C3D_E_UNSUPPORTED
        binding.sizes()   # make_plan's own refusal (a tensor too large for the narrow kernels) raises with its own message
        d = binding.desc  # else make_fold_plan's (csrc/stage_plan.h)
        raise L.Change3DHipError(
            f"the folded-BatchNorm inference path does not take the stage geometry B={d.B} T={d.T} {d.H}x{d.W}: an SE block of "
            f"up to 224 channels needs T*Ho*Wo (output rows per sample) to be a multiple of 16")
    if rc != 0:
        raise L.Change3DHipError(f"c3d_stage_fold_bytes failed with code {rc}")
    return int(a.value), int(b.value)


def stage_fold_bn(binding, fold):
    rc = L.lib().c3d_stage_fold_bn(C.byref(binding.desc), fold.data_ptr(), _stream())
    if rc != 0:
        raise L.Change3DHipError(f"c3d_stage_fold_bn failed with code {rc}")


def stage_fwd_folded(binding, fold, x, ws, y):
    rc = L.lib().c3d_stage_fwd_folded(C.byref(binding.desc), fold.data_ptr(), x.data_ptr(), ws.data_ptr(), y.data_ptr(),
                                      _stream())
    if rc != 0:
        raise L.Change3DHipError(f"c3d_stage_fwd_folded failed with code {rc}")


def stage_fwd(binding, x, ws, y):
    rc = L.lib().c3d_stage_fwd(C.byref(binding.desc), x.data_ptr(), ws.data_ptr(), y.data_ptr(), _stream())
    if rc != 0:
        raise L.Change3DHipError(f"c3d_stage_fwd failed with code {rc}")


def stage_bwd(binding, x, y, dy, ws, wb, dx):
    rc = L.lib().c3d_stage_bwd(C.byref(binding.desc), x.data_ptr(), y.data_ptr(), dy.data_ptr(), ws.data_ptr(),
                               wb.data_ptr(), dx.data_ptr(), _stream())
    if rc != 0:
        raise L.Change3DHipError(f"c3d_stage_bwd failed with code {rc}")


# ------------------------------------------------------------------------------ input pipeline
def bcd_preprocess(image6, label, flags, mean6, std6, pre, post, label_out, B, H, W):
    _launch("c3d_bcd_preprocess", B * H * W * (7 + 28), L.lib().c3d_bcd_preprocess, _p(image6), _p(label), _p(flags),
            _p(mean6), _p(std6), _p(pre), _p(post), _p(label_out), B, H, W, _stream())


def scd_label_preprocess(label3, flags, out, B, H, W):
    _launch("c3d_scd_label_preprocess", B * H * W * (3 + 24), L.lib().c3d_scd_label_preprocess, _p(label3), _p(flags), _p(out),
            B, H, W, _stream())


def bda_label_preprocess(label2, flags, label_loc, label_cls, B, H, W):
    _launch("c3d_bda_label_preprocess", B * H * W * (2 + 12), L.lib().c3d_bda_label_preprocess, _p(label2), _p(flags),
            _p(label_loc), _p(label_cls), B, H, W, _stream())


def cc_preprocess(img, swap, lut, pre, post, B, H, W):
    _launch("c3d_cc_preprocess", B * H * W * (6 + 24), L.lib().c3d_cc_preprocess, _p(img), _p(swap), _p(lut), _p(pre), _p(post),
            B, H, W, _stream())


def augment_gather(store, label_store, table, mean6, std6, pre, post, label_a, label_b, scratch, task, N, Hs, Ws, B, H, W):
    """c3d_augment_gather: one launch (two through `scratch` when a table meets a store size other than H x W).  `table` is a
    DEVICE int32 [B, 8]; validate its host copy with data.transforms.validate_augment_table before the upload."""
    lb = {L.AUG_NONE: 0, L.AUG_BCD: 1 + 4, L.AUG_SCD: 3 + 24, L.AUG_BDA: 2 + 12}[task]
    _launch("c3d_augment_gather", B * H * W * (6 + 24 + lb), L.lib().c3d_augment_gather, _p(store), _p(label_store), _p(table),
            _p(mean6), _p(std6), _p(pre), _p(post), _p(label_a), _p(label_b), _p(scratch), task, N, Hs, Ws, B, H, W, _stream())


def scene_gather(scene, origins, mean6, std6, pre, post, Hs, Ws, n, th, tw):
    """c3d_scene_gather: `n` tiles of th x tw from the resident uint8 scene [Hs, Ws, 6]; `origins` is a DEVICE int32 [n, 2]
    of (y, x), reflected where a tile overhangs."""
    _launch("c3d_scene_gather", n * th * tw * (6 + 24), L.lib().c3d_scene_gather, _p(scene), _p(origins), _p(mean6), _p(std6),
            _p(pre), _p(post), Hs, Ws, n, th, tw, _stream())


def scene_stitch(ring, wy, wx, blend, cls, Hs, Ws, C, th, tw, sy, sx, row, gate=None):
    """c3d_scene_stitch: the scene rows final after tile row `row` from the ring f32 [ky, ncols, C, th, tw] into `blend`
    (f32 [C, Hs, Ws] or None) and `cls` (u8 [Hs, Ws] or None: mask for C == 1, argmax for C > 1, times the u8 map `gate`)."""
    ky, kx = -(-th // max(sy, 1)), -(-tw // max(sx, 1))
    rows = min(sy + (th - sy) // 2, Hs)
    nbytes = rows * Ws * C * (ky * kx * 4 + (4 if blend is not None else 0)) + (rows * Ws if cls is not None else 0)
    _launch("c3d_scene_stitch", nbytes, L.lib().c3d_scene_stitch, _p(ring), _p(wy), _p(wx), _p(blend), _p(cls), _p(gate), Hs, Ws,
            C, th, tw, sy, sx, row, _stream())


def view_count(view_mask):
    """Number of views of a view mask (bit v = view code v, include/change3d_hip.h "Views"); host only."""
    return bin(int(view_mask) & 0xff).count("1")


def scene_gather_views(scene, origins, mean6, std6, pre, post, Hs, Ws, n, th, tw, view_mask):
    """c3d_scene_gather_views: `scene_gather` under every view of `view_mask`; `pre`, `post` f32 [n * nv, 3, th, tw], entry
    i * nv + j is view j (ascending code) of tile i."""
    nv = view_count(view_mask)
    if pre.numel() < n * nv * 3 * th * tw or post.numel() < n * nv * 3 * th * tw:
        raise ValueError(f"pre and post must hold {n} tiles x {nv} views of 3 x {th} x {tw}")
    _launch("c3d_scene_gather_views", n * th * tw * (6 + 24 * nv), L.lib().c3d_scene_gather_views, _p(scene), _p(origins), _p(mean6),
            _p(std6), _p(pre), _p(post), Hs, Ws, n, th, tw, int(view_mask), _stream())


def scene_fold_views(values, dst, cnt, C, th, tw, view_mask):
    """c3d_scene_fold_views: `values` f32 [cnt * nv, C, th, tw] (the model's outputs, tile-major, view-minor) -> `dst` f32
    [cnt, C, th, tw] = the mean over the views with each view undone; `dst` may be a slot range of a stitch ring."""
    nv = view_count(view_mask)
    if values.dtype != torch.float32 or dst.dtype != torch.float32 or not values.is_contiguous() or not dst.is_contiguous():
        raise ValueError("values and dst must be contiguous float32 tensors")
    if values.numel() != cnt * nv * C * th * tw or dst.numel() != cnt * C * th * tw:
        raise ValueError(f"values must hold {cnt} x {nv} and dst {cnt} entries of {C} x {th} x {tw}")
    _launch("c3d_scene_fold_views", cnt * C * th * tw * 4 * (nv + 1), L.lib().c3d_scene_fold_views, _p(values), _p(dst), cnt, C, th,
            tw, int(view_mask), _stream())


def scene_label_tile():
    """(th, tw) of the LDS tile of c3d_scene_objects' local phase; host only."""
    th, tw = C.c_int32(0), C.c_int32(0)
    L.check(L.lib().c3d_scene_label_tile(C.byref(th), C.byref(tw)), "c3d_scene_label_tile")
    return th.value, tw.value


def scene_objects(mask, cls_map=None, score=None, connectivity=8, min_area=1, n_cls=1, first_class=1, max_objects=65536,
                  want_hist=True, want_object_cls=True):
    """c3d_scene_objects on the u8 map `mask` [Hs, Ws] (nonzero = foreground): `(labels i32 [Hs, Ws], table i32 [max_objects,
    8], hist i32-holding-u32 [max_objects, n_cls] or None, object_cls u8 [Hs, Ws] or None, counts i32 [2])`, all on the
    device; nothing is read back.  `hist` exists only with a class map."""
    assert mask.dtype == torch.uint8 and mask.dim() == 2 and mask.is_contiguous() and mask.is_cuda
    Hs, Ws = int(mask.shape[0]), int(mask.shape[1])
    if cls_map is not None:
        assert cls_map.dtype == torch.uint8 and cls_map.shape == mask.shape and cls_map.is_contiguous()
    if score is not None:
        assert score.dtype == torch.float32 and score.shape == mask.shape and score.is_contiguous()
    nbytes = L.lib().c3d_scene_label_ws_bytes(Hs, Ws, int(n_cls) if cls_map is not None else 1)
    if nbytes < 0 or int(max_objects) < 1:
        raise L.Change3DHipError(f"c3d_scene_objects refuses a {Hs} x {Ws} scene with n_cls = {n_cls}, max_objects = "
                                 f"{max_objects} (code {nbytes if nbytes < 0 else -1})")
    dev = mask.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty((Hs, Ws), dtype=torch.int32, device=dev)
    table = torch.empty((int(max_objects), 8), dtype=torch.int32, device=dev)
    hist = torch.empty((int(max_objects), int(n_cls)), dtype=torch.int32, device=dev) if want_hist and cls_map is not None else None
    object_cls = torch.empty((Hs, Ws), dtype=torch.uint8, device=dev) if want_object_cls else None
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _launch("c3d_scene_objects", Hs * Ws * 40, L.lib().c3d_scene_objects, _p(mask), _p(cls_map), _p(score), Hs, Ws,
            int(connectivity), int(min_area), int(n_cls), int(first_class), int(max_objects), _p(labels), _p(table), _p(hist),
            _p(object_cls), _p(counts), _p(ws), _stream())
    return labels, table, hist, object_cls, counts


def objects_match_plan(Hs, Ws, table_capacity=0):
    """c3d_objects_match_ws_bytes: (workspace bytes, table capacity); `table_capacity` 0 asks for the one that cannot overflow."""
    cap = C.c_int64(int(table_capacity))
    nbytes = L.lib().c3d_objects_match_ws_bytes(int(Hs), int(Ws), C.byref(cap))
    if nbytes < 0:
        raise L.Change3DHipError(f"c3d_objects_match refuses a {Hs} x {Ws} scene with a table of {table_capacity} slots (code {nbytes})")
    return int(nbytes), int(cap.value)


def objects_match(labels_p, table_p, counts_p, labels_g, table_g, counts_g, n_cls=1, iou_thr=0.5, table_capacity=0, totals=None,
                  total_iou=None, ws=None):
    """c3d_objects_match on the `labels`, `table` and `counts` of two `scene_objects` calls over the same scene, prediction first:
    `(match_p i32 [max_p, 4], match_g i32 [max_g, 4], conf i64 [n_cls, n_cls], counts i64 [6], sum_iou f64 [1])`, all on the
    device; nothing is read back.  `totals` i64 [5 + n_cls * n_cls] and `total_iou` f64 [1], zeroed once by the caller, are
    added into."""
    for t in (labels_p, table_p, counts_p, labels_g, table_g, counts_g):
        require_gpu(t, "objects_match input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert labels_p.dim() == 2 and labels_g.shape == labels_p.shape and table_p.shape[1] == 8 and table_g.shape[1] == 8
    Hs, Ws = int(labels_p.shape[0]), int(labels_p.shape[1])
    max_p, max_g, n_cls = int(table_p.shape[0]), int(table_g.shape[0]), int(n_cls)
    nbytes, cap = objects_match_plan(Hs, Ws, table_capacity)
    dev = labels_p.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.numel() >= nbytes
    if totals is not None:
        assert totals.dtype == torch.int64 and totals.numel() == 5 + n_cls * n_cls and totals.is_contiguous()
    if total_iou is not None:
        assert total_iou.dtype == torch.float64 and total_iou.numel() == 1
    match_p = torch.empty((max_p, 4), dtype=torch.int32, device=dev)
    match_g = torch.empty((max_g, 4), dtype=torch.int32, device=dev)
    conf = torch.empty((max(n_cls, 1), max(n_cls, 1)), dtype=torch.int64, device=dev)   # n_cls < 1 is refused by the call
    counts = torch.empty(6, dtype=torch.int64, device=dev)
    sum_iou = torch.empty(1, dtype=torch.float64, device=dev)
    _launch("c3d_objects_match", Hs * Ws * 8 + cap * 24, L.lib().c3d_objects_match, _p(labels_p), _p(table_p), _p(counts_p),
            _p(labels_g), _p(table_g), _p(counts_g), Hs, Ws, max_p, max_g, n_cls, float(iou_thr), cap, _p(match_p), _p(match_g),
            _p(conf), _p(counts), _p(sum_iou), _p(totals), _p(total_iou), _p(ws), _stream())
    return match_p, match_g, conf, counts, sum_iou


def scene_outlines_defaults(Hs, Ws, max_objects=65536):
    """(max_rings, max_vertices) where the caller names none: 4 ring rows per table row of `scene_objects` (an outline and
    three holes each, on average) and 16 vertices per ring row, both cut to what a scene of this size can hold at all.  The
    worst case is far above either: a 4-connected checkerboard has Hs * Ws / 2 rings and 2 * Hs * Ws vertices, and a label
    map of single pixels with distinct ids has Hs * Ws rings and 4 * Hs * Ws vertices.  A scene that exceeds the defaults
    sets `OUTLINE_ST_TRUNCATED` and loses the rings past the limits, never anything else."""
    N = int(Hs) * int(Ws)
    max_rings = max(1, min(4 * int(max_objects), N))
    return max_rings, max(1, min(16 * max_rings, 4 * N))


def scene_outlines(labels, counts, connectivity=8, max_objects=65536, max_rings=None, max_vertices=None, ws=None):
    """c3d_scene_outlines on the `labels` i32 [Hs, Ws] and `counts` i32 [2] of `scene_objects` (same `connectivity` and
    `max_objects`): `(rings i32 [max_rings, 8] = (id, start, n_vertices, area, perimeter, x, y, 0), vertices i32 [max_vertices,
    2] = (vx, vy), counts i32 [5] = (rings found, rows written, vertices found, vertices written, status))`, all on the
    device; nothing is read back.  Vertex rows past counts[3] are not initialised.  Defaults: `scene_outlines_defaults`."""
    for t in (labels, counts):
        require_gpu(t, "scene_outlines input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert labels.dim() == 2 and counts.numel() == 2
    Hs, Ws = int(labels.shape[0]), int(labels.shape[1])
    d_rings, d_vertices = scene_outlines_defaults(Hs, Ws, max_objects)
    max_rings = d_rings if max_rings is None else int(max_rings)
    max_vertices = d_vertices if max_vertices is None else int(max_vertices)
    nbytes = L.lib().c3d_scene_outlines_ws_bytes(Hs, Ws)
    if nbytes < 0 or int(max_objects) < 1 or max_rings < 1 or max_vertices < 1 or connectivity not in (4, 8):
        raise L.Change3DHipError(f"c3d_scene_outlines refuses a {Hs} x {Ws} scene with connectivity = {connectivity}, max_objects = "
                                 f"{max_objects}, max_rings = {max_rings}, max_vertices = {max_vertices} (code "
                                 f"{nbytes if nbytes < 0 else -1})")
    dev = labels.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    rings = torch.empty((max_rings, 8), dtype=torch.int32, device=dev)
    vertices = torch.empty((max_vertices, 2), dtype=torch.int32, device=dev)
    out = torch.empty(5, dtype=torch.int32, device=dev)
    _launch("c3d_scene_outlines", Hs * Ws * 64, L.lib().c3d_scene_outlines, _p(labels), _p(counts), Hs, Ws, int(connectivity),
            int(max_objects), max_rings, max_vertices, _p(rings), _p(vertices), _p(out), _p(ws), _stream())
    return rings, vertices, out


def simplify_tol2_q(tol):
    """The tolerance of `outlines_simplify` as the call takes it: round(16 * tol * tol), sixteenths of a square pixel.  Raises
    outside [0, 1024] pixels."""
    tol = float(tol)
    if not 0.0 <= tol <= 1024.0:                          # also refuses NaN
        raise ValueError(f"the simplification tolerance must lie in [0, 1024] pixels, got {tol}")
    return int(round(16.0 * tol * tol))


def outlines_simplify_limits():
    """(most vertices of a ring that one wave simplifies, most of a ring that one workgroup keeps in LDS)."""
    out = (L.C.c_int32 * 2)()
    L.lib().c3d_outlines_simplify_limits(out)
    return int(out[0]), int(out[1])


def outlines_simplify(rings, vertices, counts, tol, ws=None):
    """c3d_outlines_simplify on the `rings` i32 [max_rings, 8], `vertices` i32 [max_vertices, 2] and `counts` i32 [5] of
    `scene_outlines` (or any table of that shape): Douglas-Peucker with the tolerance `tol` in pixels, by the integer rule of
    include/change3d_hip.h.  Returns `(rings_out i32 [max_rings, 8] = (id, start', n', area2', perimeter, x, y, n),
    vertices_out i32 [max_vertices, 2], counts_out i32 [5] = (rings found, rows written, vertices kept, vertices written,
    status))`, all on the device; nothing is read back.  Vertex rows past counts_out[3] are not initialised."""
    tol2_q = simplify_tol2_q(tol)
    for t in (rings, vertices, counts):
        require_gpu(t, "outlines_simplify input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    max_rings, max_vertices = int(rings.shape[0]), int(vertices.shape[0])
    nbytes = L.lib().c3d_outlines_simplify_ws_bytes(max_rings, max_vertices)
    if nbytes < 0:
        raise L.Change3DHipError(f"c3d_outlines_simplify refuses max_rings = {max_rings}, max_vertices = {max_vertices} (code {nbytes})")
    dev = rings.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    rings_out = torch.empty((max_rings, 8), dtype=torch.int32, device=dev)
    vertices_out = torch.empty((max_vertices, 2), dtype=torch.int32, device=dev)
    out = torch.empty(5, dtype=torch.int32, device=dev)
    _launch("c3d_outlines_simplify", (max_rings + max_vertices) * 64, L.lib().c3d_outlines_simplify, _p(rings), _p(vertices),
            _p(counts), max_rings, max_vertices, tol2_q, _p(rings_out), _p(vertices_out), _p(out), _p(ws), _stream())
    return rings_out, vertices_out, out


def outlines_simplify_shared_limits():
    """(most augmented vertices of a ring that one wave simplifies, most of a ring whose state one workgroup keeps in LDS)."""
    out = (L.C.c_int32 * 2)()
    L.lib().c3d_outlines_simplify_shared_limits(out)
    return int(out[0]), int(out[1])


def outlines_simplify_shared(labels, counts_obj, rings, vertices, counts, tol, max_objects=65536, max_vertices_out=None, ws=None):
    """c3d_outlines_simplify_shared on the `labels` i32 [Hs, Ws] and `counts_obj` i32 [2] of `scene_objects` / `scene_split` and the
    `rings`, `vertices` and `counts` that `scene_outlines` wrote for them: every wall between two objects is cut at the points
    where three or more regions meet and simplified once for both neighbours, with the tolerance `tol` in pixels, by the integer
    rule of include/change3d_hip.h.  Returns `(rings_out i32 [max_rings, 8] = (id, start', n', area2', perimeter, x', y', n),
    vertices_out i32 [max_vertices_out, 2], counts_out i32 [5], left i32 [max_vertices_out] = the label left of the edge that
    leaves each vertex, info i32 [8] = (nodes inserted, node vertices, arcs, closed arcs, arcs with a neighbour, collapsed rings,
    0, 0))`, all on the device; nothing is read back.  `max_vertices_out` defaults to twice the rows of `vertices`, which
    always suffices for a complete table.  Vertex and left rows past counts_out[3] are not initialised."""
    tol2_q = simplify_tol2_q(tol)
    for t in (labels, counts_obj, rings, vertices, counts):
        require_gpu(t, "outlines_simplify_shared input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert labels.dim() == 2 and counts_obj.numel() == 2
    assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    Hs, Ws = int(labels.shape[0]), int(labels.shape[1])
    max_rings, max_vertices = int(rings.shape[0]), int(vertices.shape[0])
    max_out = 2 * max_vertices if max_vertices_out is None else int(max_vertices_out)
    nbytes = L.lib().c3d_outlines_simplify_shared_ws_bytes(Hs, Ws, max_rings, max_vertices)
    if nbytes < 0 or max_out < 1 or int(max_objects) < 1:
        raise L.Change3DHipError(f"c3d_outlines_simplify_shared refuses a {Hs} x {Ws} scene with max_objects = {max_objects}, max_rings = "
                                 f"{max_rings}, max_vertices = {max_vertices}, max_vertices_out = {max_out} (code "
                                 f"{nbytes if nbytes < 0 else -1})")
    dev = rings.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    rings_out = torch.empty((max_rings, 8), dtype=torch.int32, device=dev)
    vertices_out = torch.empty((max_out, 2), dtype=torch.int32, device=dev)
    left = torch.empty(max_out, dtype=torch.int32, device=dev)
    out = torch.empty(5, dtype=torch.int32, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    _launch("c3d_outlines_simplify_shared", (max_rings + max_vertices) * 128, L.lib().c3d_outlines_simplify_shared, _p(labels),
            _p(counts_obj), Hs, Ws, int(max_objects), _p(rings), _p(vertices), _p(counts), max_rings, max_vertices, tol2_q, max_out,
            _p(rings_out), _p(vertices_out), _p(left), _p(out), _p(info), _p(ws), _stream())
    return rings_out, vertices_out, out, left, info


def outlines_simplify_safe_limits():
    """(the two tier limits of the Douglas-Peucker as in `outlines_simplify_shared_limits`, most entries of a cell in the detector's
    wave tier, entries of a chunk, entry budget and cell budget per live edge); host only."""
    out = (C.c_int32 * 6)()
    L.lib().c3d_outlines_simplify_safe_limits(out)
    return tuple(int(v) for v in out)


def outlines_simplify_safe(labels, counts_obj, rings, vertices, counts, tol, max_rounds=8, max_work=2 ** 32, max_objects=65536,
                           max_vertices_out=None, ws=None):
    """c3d_outlines_simplify_safe: `outlines_simplify_shared` in rounds with a tolerance per arc.  The arcs that take part in a
    defect of the output (two edges that cross or overlap, a vertex inside another edge, a ring that collapsed or flipped) get a
    quarter of their squared tolerance and every ring is simplified again, until a round finds nothing or `max_rounds` rounds
    have run, by the integer rule of include/change3d_hip.h.  Returns `(rings_out, vertices_out, counts_out, left, info, level,
    safe)`: the first five as `outlines_simplify_shared` returns them (info[6], info[7] = the shift and the work of the last
    round's grid), `level` i32 [max_vertices_out] = the level of the arc of the edge that leaves each vertex, `safe` i64 [8] =
    (rounds run, rounds that raised, arcs with level > 0, arcs at the cap, defective pairs in round 0, in the last round,
    defective rings in round 0, status: 0 converged, 1 not converged, 2 defects left, 3 over `max_work`).  All on the device;
    nothing is read back, the rounds are launched ahead."""
    tol2_q = simplify_tol2_q(tol)
    for t in (labels, counts_obj, rings, vertices, counts):
        require_gpu(t, "outlines_simplify_safe input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert labels.dim() == 2 and counts_obj.numel() == 2
    assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    if not 1 <= int(max_rounds) <= 64:
        raise ValueError(f"max_rounds = {max_rounds} is outside [1, 64]")
    if int(max_work) < 0:
        raise ValueError(f"max_work = {max_work} is negative")
    Hs, Ws = int(labels.shape[0]), int(labels.shape[1])
    max_rings, max_vertices = int(rings.shape[0]), int(vertices.shape[0])
    max_out = 2 * max_vertices if max_vertices_out is None else int(max_vertices_out)
    nbytes = L.lib().c3d_outlines_simplify_safe_ws_bytes(Hs, Ws, max_rings, max_vertices, max_out) if max_out >= 1 else -1
    if nbytes < 0 or int(max_objects) < 1:
        raise L.Change3DHipError(f"c3d_outlines_simplify_safe refuses a {Hs} x {Ws} scene with max_objects = {max_objects}, max_rings = "
                                 f"{max_rings}, max_vertices = {max_vertices}, max_vertices_out = {max_out} (code {min(nbytes, -1)})")
    dev = rings.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    rings_out = torch.empty((max_rings, 8), dtype=torch.int32, device=dev)
    vertices_out = torch.empty((max_out, 2), dtype=torch.int32, device=dev)
    left = torch.empty(max_out, dtype=torch.int32, device=dev)
    level = torch.empty(max_out, dtype=torch.int32, device=dev)
    out = torch.empty(5, dtype=torch.int32, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    safe = torch.empty(8, dtype=torch.int64, device=dev)
    _launch("c3d_outlines_simplify_safe", (max_rings + max_vertices) * 128, L.lib().c3d_outlines_simplify_safe, _p(labels),
            _p(counts_obj), Hs, Ws, int(max_objects), _p(rings), _p(vertices), _p(counts), max_rings, max_vertices, tol2_q, int(max_rounds),
            int(max_work), max_out, _p(rings_out), _p(vertices_out), _p(left), _p(level), _p(out), _p(info), _p(safe), _p(ws), _stream())
    return rings_out, vertices_out, out, left, info, level, safe


def rings_fill_limits():
    """(most rows and columns of an id's pixel box that one wave fills, rows of a band of a larger box); host only."""
    out = (C.c_int32 * 2)()
    L.lib().c3d_rings_fill_limits(out)
    return int(out[0]), int(out[1])


def rings_fill(rings, vertices, counts, Hs, Ws, frac_bits=0, id_cls=None, max_objects=65536, want_mask=False, want_cls_map=False,
               ws=None):
    """c3d_rings_fill on the `rings` i32 [max_rings, 8], `vertices` i32 [max_vertices, 2] and `counts` i32 [5] of
    `scene_outlines` / `outlines_simplify` (or any table of that shape, coordinates in units of 2^-frac_bits pixel): the
    polygons filled into an Hs x Ws label map by the integer rule of include/change3d_hip.h -- centre sampling, even-odd per
    id, the largest id wins.  Returns `(labels i32 [Hs, Ws], table i32 [max_objects, 8] in `scene_objects`' row format,
    counts_obj i32 [2] = (K, K), mask u8 [Hs, Ws] or None, cls_map u8 [Hs, Ws] or None, info i32 [4] = (status, ring rows
    used, K, 0))`, all on the device; nothing is read back.  `id_cls` u8 [max_objects] gives every id its class."""
    for t in (rings, vertices, counts):
        require_gpu(t, "rings_fill input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    max_rings, max_vertices, max_objects = int(rings.shape[0]), int(vertices.shape[0]), int(max_objects)
    Hs, Ws, frac_bits = int(Hs), int(Ws), int(frac_bits)
    if not 0 <= frac_bits <= 8:
        raise ValueError(f"frac_bits must lie in [0, 8], got {frac_bits}")
    nbytes = L.lib().c3d_rings_fill_ws_bytes(max_rings, max_vertices, max_objects, Hs, Ws)
    if nbytes < 0:
        raise L.Change3DHipError(f"c3d_rings_fill refuses a {Hs} x {Ws} scene with max_rings = {max_rings}, max_vertices = "
                                 f"{max_vertices}, max_objects = {max_objects} (code {nbytes})")
    dev = rings.device
    if id_cls is not None:
        require_gpu(id_cls, "rings_fill id_cls")
        assert id_cls.dtype == torch.uint8 and id_cls.numel() == max_objects and id_cls.is_contiguous() and id_cls.device == dev
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    labels = torch.empty((Hs, Ws), dtype=torch.int32, device=dev)
    table = torch.empty((max_objects, 8), dtype=torch.int32, device=dev)
    counts_obj = torch.empty(2, dtype=torch.int32, device=dev)
    mask = torch.empty((Hs, Ws), dtype=torch.uint8, device=dev) if want_mask else None
    cls_map = torch.empty((Hs, Ws), dtype=torch.uint8, device=dev) if want_cls_map else None
    info = torch.empty(4, dtype=torch.int32, device=dev)
    _launch("c3d_rings_fill", Hs * Ws * 10 + (max_rings + max_vertices) * 16, L.lib().c3d_rings_fill, _p(rings), _p(vertices),
            _p(counts), max_rings, max_vertices, frac_bits, _p(id_cls), max_objects, Hs, Ws, _p(labels), _p(table), _p(counts_obj),
            _p(mask), _p(cls_map), _p(info), _p(ws), _stream())
    return labels, table, counts_obj, mask, cls_map, info


def rings_hull_limits():
    """(most points of an id that one wave keeps in registers, most points of an id whose candidates one workgroup is sure
    to keep in LDS); host only."""
    out = (C.c_int32 * 2)()
    L.lib().c3d_rings_hull_limits(out)
    return int(out[0]), int(out[1])


def rings_hull(rings, vertices, counts, max_objects=65536, max_hull_vertices=None, ws=None):
    """c3d_rings_hull on the `rings` i32 [max_rings, 8], `vertices` i32 [max_vertices, 2] and `counts` i32 [5] of
    `scene_outlines` (or any table of that shape with integer pixel corners): the strictly convex hull and the minimum-area
    rectangle of every id, by the integer rule of include/change3d_hip.h.  Returns `(hulls i32 [max_objects, 8] = (id, start,
    m, area2, 0, x, y, n_points), hull_vertices i32 [max_hull_vertices, 2], rects i64 [max_objects, 8] = (k, L, t_min, t_max,
    c_max, j_tmin, j_tmax, j_cmax), counts_out i32 [5] = (ids with points, K, hull vertices found, written, status))`, all on
    the device; nothing is read back.  `max_hull_vertices` defaults to `vertices.shape[0]`, which never truncates a table
    whose rows share no vertices.  Vertex rows past counts_out[3] are not initialised."""
    for t in (rings, vertices, counts):
        require_gpu(t, "rings_hull input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    max_rings, max_vertices, max_objects = int(rings.shape[0]), int(vertices.shape[0]), int(max_objects)
    max_hull_vertices = max_vertices if max_hull_vertices is None else int(max_hull_vertices)
    nbytes = L.lib().c3d_rings_hull_ws_bytes(max_rings, max_vertices, max_objects)
    if nbytes < 0 or max_hull_vertices < 1:
        raise L.Change3DHipError(f"c3d_rings_hull refuses max_rings = {max_rings}, max_vertices = {max_vertices}, max_objects = "
                                 f"{max_objects}, max_hull_vertices = {max_hull_vertices} (code {nbytes if nbytes < 0 else -1})")
    dev = rings.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    hulls = torch.empty((max_objects, 8), dtype=torch.int32, device=dev)
    hull_vertices = torch.empty((max_hull_vertices, 2), dtype=torch.int32, device=dev)
    rects = torch.empty((max_objects, 8), dtype=torch.int64, device=dev)
    out = torch.empty(5, dtype=torch.int32, device=dev)
    _launch("c3d_rings_hull", (max_rings + max_vertices) * 32 + max_objects * 120, L.lib().c3d_rings_hull, _p(rings), _p(vertices),
            _p(counts), max_rings, max_vertices, max_objects, max_hull_vertices, _p(hulls), _p(hull_vertices), _p(rects), _p(out),
            _p(ws), _stream())
    return hulls, hull_vertices, rects, out


def rings_regularize_limits():
    """(most edges of a ring that one wave regularises, most of a ring whose state one workgroup keeps in LDS); host only."""
    out = (C.c_int32 * 2)()
    L.lib().c3d_rings_regularize_limits(out)
    return int(out[0]), int(out[1])


def rings_regularize(rings, vertices, counts, hulls, hull_vertices, rects, hull_counts, frac_bits=4, ws=None):
    """c3d_rings_regularize on the `rings` i32 [max_rings, 8], `vertices` i32 [max_vertices, 2] and `counts` i32 [5] of
    `outlines_simplify` (or any table of that shape with integer pixel corners) and the four outputs of `rings_hull` for the
    same ids: every ring squared to the axes of its id's minimum-area rectangle by the integer rule of
    include/change3d_hip.h.  Returns `(rings_out i32 [max_rings, 8] = (id, start', n', flag, perimeter, x, y, n), vertices_out
    i32 [max_vertices, 2] in units of 2^-frac_bits pixel, counts_out i32 [5] = (rings found, rows written, vertices out,
    vertices out, status))`, all on the device; nothing is read back.  `rings_fill(..., frac_bits=frac_bits)` takes them as
    they are.  Vertex rows past counts_out[3] are not initialised."""
    for t in (rings, vertices, counts, hulls, hull_vertices, hull_counts):
        require_gpu(t, "rings_regularize input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    require_gpu(rects, "rings_regularize input")
    assert rects.dtype == torch.int64 and rects.is_contiguous()
    assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    assert hulls.dim() == 2 and hulls.shape[1] == 8 and tuple(rects.shape) == tuple(hulls.shape)
    assert hull_vertices.dim() == 2 and hull_vertices.shape[1] == 2 and hull_counts.numel() == 5
    max_rings, max_vertices = int(rings.shape[0]), int(vertices.shape[0])
    max_objects, max_hull_vertices, frac_bits = int(hulls.shape[0]), int(hull_vertices.shape[0]), int(frac_bits)
    if not 0 <= frac_bits <= 8:
        raise ValueError(f"frac_bits must lie in [0, 8], got {frac_bits}")
    nbytes = L.lib().c3d_rings_regularize_ws_bytes(max_rings, max_vertices, max_objects)
    if nbytes < 0 or max_hull_vertices < 1:
        raise L.Change3DHipError(f"c3d_rings_regularize refuses max_rings = {max_rings}, max_vertices = {max_vertices}, max_objects "
                                 f"= {max_objects}, max_hull_vertices = {max_hull_vertices} (code {nbytes if nbytes < 0 else -1})")
    dev = rings.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    rings_out = torch.empty((max_rings, 8), dtype=torch.int32, device=dev)
    vertices_out = torch.empty((max_vertices, 2), dtype=torch.int32, device=dev)
    out = torch.empty(5, dtype=torch.int32, device=dev)
    _launch("c3d_rings_regularize", (max_rings + max_vertices) * 48, L.lib().c3d_rings_regularize, _p(rings), _p(vertices),
            _p(counts), max_rings, max_vertices, _p(hulls), _p(hull_vertices), _p(rects), _p(hull_counts), max_objects,
            max_hull_vertices, frac_bits, _p(rings_out), _p(vertices_out), _p(out), _p(ws), _stream())
    return rings_out, vertices_out, out


def rings_polis_limits():
    """(most vertices of either id in the wave tier, vertices of a job, edges of an LDS tile, most rings of an id, most vertices
    of a ring that one wave regroups); host only."""
    out = (C.c_int32 * 5)()
    L.lib().c3d_rings_polis_limits(out)
    return tuple(int(v) for v in out)


def rings_polis(rings_p, vertices_p, counts_p, frac_bits_p, rings_g, vertices_g, counts_g, frac_bits_g, match_p, max_g,
                max_pair_work=2 ** 32, totals=None, total_sums=None, ws=None):
    """c3d_rings_polis on two ring tables (`rings` i32 [max_rings, 8], `vertices` i32 [max_vertices, 2], `counts` i32 [5],
    coordinates in units of 2^-frac_bits pixel), prediction first, and the `match_p` i32 [max_p, 4] of `objects_match`: PoLiS
    and the vertex-to-boundary Hausdorff distance of every matched pair by the rule of include/change3d_hip.h.  Returns `(pair
    f64 [max_p, 4] = (polis, hausdorff, mean_pg, mean_gp) in pixels, pair_n i32 [max_p, 4] = (g, n_p, n_g, flag), counts i64
    [8] = (scored, no partner, incomplete, over work, sum n_p, sum n_g, status, 0), sums f64 [4] = (sum polis, sum hausdorff,
    max hausdorff, sum n_p / n_g))`, all on the device; nothing is read back.  `totals` i64 [8] and `total_sums` f64 [4],
    zeroed once by the caller, are accumulated into.  A pair that would cost more than `max_pair_work` point-edge
    evaluations is not scored (flag 3)."""
    for t in (rings_p, vertices_p, counts_p, rings_g, vertices_g, counts_g, match_p):
        require_gpu(t, "rings_polis input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    for rings, vertices, counts in ((rings_p, vertices_p, counts_p), (rings_g, vertices_g, counts_g)):
        assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    assert match_p.dim() == 2 and match_p.shape[1] == 4
    frac_bits_p, frac_bits_g, max_pair_work = int(frac_bits_p), int(frac_bits_g), int(max_pair_work)
    if not (0 <= frac_bits_p <= 8 and 0 <= frac_bits_g <= 8):
        raise ValueError(f"frac_bits must lie in [0, 8], got {frac_bits_p} and {frac_bits_g}")
    if not 0 <= max_pair_work < 2 ** 63:
        raise ValueError(f"max_pair_work must lie in [0, 2^63), got {max_pair_work}")
    sizes = (int(rings_p.shape[0]), int(vertices_p.shape[0]), int(match_p.shape[0]), int(rings_g.shape[0]),
             int(vertices_g.shape[0]), int(max_g))
    nbytes = L.lib().c3d_rings_polis_ws_bytes(*sizes)
    if nbytes < 0:
        raise L.Change3DHipError(f"c3d_rings_polis refuses (max_rings, max_vertices, max_objects) = {sizes[:3]} against {sizes[3:]} "
                                 f"(code {nbytes})")
    dev = rings_p.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    if totals is not None:
        require_gpu(totals, "rings_polis totals")
        assert totals.dtype == torch.int64 and totals.numel() == 8 and totals.is_contiguous()
    if total_sums is not None:
        require_gpu(total_sums, "rings_polis total_sums")
        assert total_sums.dtype == torch.float64 and total_sums.numel() == 4 and total_sums.is_contiguous()
    max_p = sizes[2]
    pair = torch.empty((max_p, 4), dtype=torch.float64, device=dev)
    pair_n = torch.empty((max_p, 4), dtype=torch.int32, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    _launch("c3d_rings_polis", (sizes[0] + sizes[3]) * 48 + (sizes[1] + sizes[4]) * 40 + max_p * 64, L.lib().c3d_rings_polis,
            _p(rings_p), _p(vertices_p), _p(counts_p), sizes[0], sizes[1], frac_bits_p, _p(rings_g), _p(vertices_g), _p(counts_g),
            sizes[3], sizes[4], frac_bits_g, _p(match_p), max_p, sizes[5], max_pair_work, _p(pair), _p(pair_n), _p(counts),
            _p(sums), _p(totals), _p(total_sums), _p(ws), _stream())
    return pair, pair_n, counts, sums


def rings_valid_limits():
    """(most edges of an id in the wave tier, edges of a chunk, edges of an LDS tile, most rings of an id, most vertices of a
    ring that one wave regroups); host only."""
    out = (C.c_int32 * 5)()
    L.lib().c3d_rings_valid_limits(out)
    return tuple(int(v) for v in out)


def rings_valid(rings, vertices, counts, frac_bits=0, max_objects=65536, max_id_work=2 ** 32, totals=None, ws=None):
    """c3d_rings_valid on one ring table (`rings` i32 [max_rings, 8], `vertices` i32 [max_vertices, 2], `counts` i32 [5],
    coordinates in units of 2^-frac_bits pixel): the crossings, overlaps and touches among the edges of every object id by the
    rule of include/change3d_hip.h.  Returns `(valid i64 [max_objects, 8] = (flag, rings, m, degenerate, cross, overlap,
    touch_vv, touch_ve) per id, counts i64 [8] = (checked, invalid, empty, incomplete, over work, sum cross, sum overlap,
    status))`, both on the device; nothing is read back.  An id is valid iff flag == 0 and cross == overlap == 0.  `totals` i64
    [8], zeroed once by the caller, is accumulated into.  An id whose m (m - 1) / 2 edge pairs exceed `max_id_work` is not
    checked (flag 3)."""
    for t in (rings, vertices, counts):
        require_gpu(t, "rings_valid input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    frac_bits, max_objects, max_id_work = int(frac_bits), int(max_objects), int(max_id_work)
    if not 0 <= frac_bits <= 8:
        raise ValueError(f"frac_bits must lie in [0, 8], got {frac_bits}")
    if not 0 <= max_id_work < 2 ** 63:
        raise ValueError(f"max_id_work must lie in [0, 2^63), got {max_id_work}")
    max_rings, max_vertices = int(rings.shape[0]), int(vertices.shape[0])
    nbytes = L.lib().c3d_rings_valid_ws_bytes(max_rings, max_vertices, max_objects) if max_objects < 2 ** 31 else -1
    if nbytes < 0:
        raise L.Change3DHipError(f"c3d_rings_valid refuses max_rings = {max_rings}, max_vertices = {max_vertices}, max_objects = "
                                 f"{max_objects} (code {nbytes})")
    dev = rings.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    if totals is not None:
        require_gpu(totals, "rings_valid totals")
        assert totals.dtype == torch.int64 and totals.numel() == 8 and totals.is_contiguous()
    valid = torch.empty((max_objects, 8), dtype=torch.int64, device=dev)
    out = torch.empty(8, dtype=torch.int64, device=dev)
    _launch("c3d_rings_valid", max_rings * 48 + max_vertices * 56 + max_objects * 128, L.lib().c3d_rings_valid, _p(rings),
            _p(vertices), _p(counts), max_rings, max_vertices, frac_bits, max_objects, max_id_work, _p(valid), _p(out), _p(totals),
            _p(ws), _stream())
    return valid, out


def rings_conflicts_limits():
    """(most entries of a cell in the wave tier, entries of a chunk, entries of an LDS tile, most rings of an id, entries the
    grid may hold per vertex of max_vertices, cells it may have per vertex); host only."""
    out = (C.c_int32 * 6)()
    L.lib().c3d_rings_conflicts_limits(out)
    return tuple(int(v) for v in out)


def rings_conflicts(rings, vertices, counts, frac_bits=0, max_objects=65536, max_work=2 ** 32, totals=None, ws=None):
    """c3d_rings_conflicts on one ring table (`rings` i32 [max_rings, 8], `vertices` i32 [max_vertices, 2], `counts` i32 [5],
    coordinates in units of 2^-frac_bits pixel): the crossings, collinear overlaps and touches between the edges of DIFFERENT
    object ids by the rule of include/change3d_hip.h, found through a grid of edge cells built on the device.  Returns
    `(conflict i64 [max_objects, 8] = (flag, partner, m, cross, same, opposite, touch_vv, touch_ve) per id, counts i64 [8] =
    (checked, in conflict, empty, incomplete, over work, sum cross, sum same, status), info i64 [8] = (live edges, cell shift,
    cells_x, cells_y, entries, work, sum opposite, sum touches))`, all on the device; nothing is read back.  An id is in
    conflict iff flag == 0 and cross + same > 0.  `totals` i64 [8], zeroed once by the caller, is accumulated into.  If the
    grid's `work` (candidate pairs) exceeds `max_work`, no pair is evaluated (flag 3)."""
    for t in (rings, vertices, counts):
        require_gpu(t, "rings_conflicts input")
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert rings.dim() == 2 and rings.shape[1] == 8 and vertices.dim() == 2 and vertices.shape[1] == 2 and counts.numel() == 5
    frac_bits, max_objects, max_work = int(frac_bits), int(max_objects), int(max_work)
    if not 0 <= frac_bits <= 8:
        raise ValueError(f"frac_bits must lie in [0, 8], got {frac_bits}")
    if not 0 <= max_work < 2 ** 63:
        raise ValueError(f"max_work must lie in [0, 2^63), got {max_work}")
    max_rings, max_vertices = int(rings.shape[0]), int(vertices.shape[0])
    nbytes = L.lib().c3d_rings_conflicts_ws_bytes(max_rings, max_vertices, max_objects) if max_objects < 2 ** 31 else -1
    if nbytes < 0:
        raise L.Change3DHipError(f"c3d_rings_conflicts refuses max_rings = {max_rings}, max_vertices = {max_vertices}, "
                                 f"max_objects = {max_objects} (code {nbytes})")
    dev = rings.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    if totals is not None:
        require_gpu(totals, "rings_conflicts totals")
        assert totals.dtype == torch.int64 and totals.numel() == 8 and totals.is_contiguous()
    conflict = torch.empty((max_objects, 8), dtype=torch.int64, device=dev)
    out = torch.empty(8, dtype=torch.int64, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    _launch("c3d_rings_conflicts", max_rings * 40 + max_vertices * 100 + max_objects * 96, L.lib().c3d_rings_conflicts, _p(rings),
            _p(vertices), _p(counts), max_rings, max_vertices, frac_bits, max_objects, max_work, _p(conflict), _p(out), _p(info),
            _p(totals), _p(ws), _stream())
    return conflict, out, info


def rect_corners(P, d, rect_row):
    """The rectangle of a `rings_hull` rects row on the hull edge that starts at `P` = (x, y) and runs along `d` = (dx, dy):
    `(corners float64 [4, 2], long, short, angle)`.  The corners are P + d t/L (+ n c_max/L) for t = t_min, t_max with n =
    (-d.y, d.x), in the order (t_min, 0), (t_max, 0), (t_max, c_max), (t_min, c_max); long and short are the side lengths in
    pixels; angle is the direction of the long side in image coordinates (y down), in degrees in [0, 180), the side along d
    where the two are equal.  Host only."""
    import numpy as np
    k, Lq, t0, t1, c = (int(v) for v in list(rect_row)[:5])
    dx, dy = int(d[0]), int(d[1])
    if k < 0 or Lq <= 0 or dx * dx + dy * dy != Lq:
        raise ValueError("rect_corners needs a rects row with k >= 0 and the edge vector it was made on")
    x0, y0, nx, ny = float(P[0]), float(P[1]), -dy, dx
    corners = np.array([[x0 + (dx * t + nx * s) / Lq, y0 + (dy * t + ny * s) / Lq] for t, s in ((t0, 0), (t1, 0), (t1, c), (t0, c))],
                       dtype=np.float64)
    along, across = (t1 - t0) / math.sqrt(Lq), c / math.sqrt(Lq)
    ax, ay = (dx, dy) if t1 - t0 >= c else (nx, ny)        # compared as integers: both share the divisor
    angle = math.degrees(math.atan2(ay, ax)) % 180.0
    return corners, max(along, across), min(along, across), angle


def scene_edt_tile():
    """(rows of a chunk of c3d_scene_edt's column pass, pixels of a row per workgroup of its row pass); host only."""
    out = (C.c_int32 * 2)()
    L.check(L.lib().c3d_scene_edt_tile(out), "c3d_scene_edt_tile")
    return int(out[0]), int(out[1])


def _u8_map(t, what):
    require_gpu(t, what)
    if t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous u8 [Hs, Ws] map, got {t.dtype} {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1])


def _scene_ws(ws, nbytes, dev, what, Hs, Ws):
    if nbytes < 0:
        raise L.Change3DHipError(f"{what} refuses a {Hs} x {Ws} scene (code {nbytes})")
    if ws is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_cuda
    return ws


def scene_edt(mask, invert=False, border=False, cap2=0, out=None, ws=None):
    """c3d_scene_edt on the u8 map `mask` [Hs, Ws]: `dist2` i32 [Hs, Ws], the exact squared Euclidean distance of every pixel to
    the nearest site -- the zero pixels, the nonzero ones with `invert`, and everything outside the scene with `border`.
    `cap2` > 0: values above it come out as `EDT_FAR`.  On the device; nothing is read back."""
    Hs, Ws = _u8_map(mask, "scene_edt mask")
    cap2 = int(cap2)
    if not 0 <= cap2 < 2 ** 31:
        raise ValueError(f"cap2 must lie in [0, 2^31), got {cap2}")
    ws = _scene_ws(ws, L.lib().c3d_scene_edt_ws_bytes(Hs, Ws), mask.device, "c3d_scene_edt", Hs, Ws)
    if out is None:
        out = torch.empty((Hs, Ws), dtype=torch.int32, device=mask.device)
    assert out.dtype == torch.int32 and out.shape == mask.shape and out.is_contiguous() and out.device == mask.device
    flags = (L.EDT_INVERT if invert else 0) | (L.EDT_BORDER if border else 0)
    _launch("c3d_scene_edt", Hs * Ws * 9, L.lib().c3d_scene_edt, _p(mask), Hs, Ws, flags, cap2, _p(out), _p(ws), _stream())
    return out


def boundary_radius2(r):
    """A radius in pixels as `boundary_counts` takes it: floor(r * r) -- on the lattice dist <= r iff dist2 <= floor(r^2).
    Raises outside (0, 1024].  A radius below 1 gives 0, a band that holds no pixel, which `boundary_counts` refuses."""
    r = float(r)
    if not 0.0 < r <= 1024.0:                             # also refuses NaN
        raise ValueError(f"a boundary radius must lie in (0, 1024] pixels, got {r}")
    return int(math.floor(r * r))


def boundary_counts(pred, gt, d, tau=None, border=True, totals=None, ws=None):
    """c3d_boundary_counts on two u8 maps [Hs, Ws] (nonzero = object): `counts` i64 [8] = (|Pd and Gd|, |Pd or Gd|, |Pc|, hits of
    Pc, |Gc|, hits of Gc, 1, 0) for the band width `d` and the contour tolerance `tau` (default `d`), both in pixels; `border`:
    the outside of the scene counts as background.  `totals` i64 [8], zeroed once by the caller, is added into.  On the device;
    nothing is read back."""
    d2 = boundary_radius2(d)
    tau2 = d2 if tau is None else boundary_radius2(tau)
    if d2 < 1 or tau2 < 1:
        raise ValueError(f"d and tau must be at least 1 pixel: no lattice distance above 0 is smaller; got {d}, {tau}")
    Hs, Ws = _u8_map(pred, "boundary_counts prediction")
    if _u8_map(gt, "boundary_counts ground truth") != (Hs, Ws) or gt.device != pred.device:
        raise ValueError(f"the prediction is {Hs} x {Ws} on {pred.device}, the ground truth {tuple(gt.shape)} on {gt.device}")
    ws = _scene_ws(ws, L.lib().c3d_boundary_counts_ws_bytes(Hs, Ws), pred.device, "c3d_boundary_counts", Hs, Ws)
    if totals is not None:
        assert totals.dtype == torch.int64 and totals.numel() == 8 and totals.is_contiguous() and totals.device == pred.device
    counts = torch.empty(8, dtype=torch.int64, device=pred.device)
    _launch("c3d_boundary_counts", Hs * Ws * 40, L.lib().c3d_boundary_counts, _p(pred), _p(gt), Hs, Ws, d2, tau2,
            L.EDT_BORDER if border else 0, _p(counts), _p(totals), _p(ws), _stream())
    return counts


def scene_split_tile():
    """(rows, columns) of the tile that one workgroup of c3d_scene_split's growth relaxes in LDS; host only."""
    out = (C.c_int32 * 2)()
    L.check(L.lib().c3d_scene_split_tile(out), "c3d_scene_split_tile")
    return int(out[0]), int(out[1])


def scene_split(mask, r, cls_map=None, score=None, connectivity=8, min_area=1, n_cls=1, first_class=1, max_objects=65536,
                max_rounds=32, want_hist=True, want_object_cls=True, ws=None):
    """c3d_scene_split on the u8 map `mask` [Hs, Ws]: `scene_objects` with every component cut into the pieces that are joined
    by necks narrower than the radius `r` in pixels (`boundary_radius2`: r2 = floor(r * r); r = 0 splits nothing and equals
    `scene_objects`).  Returns `scene_objects`' tuple plus `info` i32 [4] = (status, seeds, rounds used, 0), all on the
    device; nothing is read back.  A status with `SPLIT_ST_NOT_CONVERGED` asks for a larger `max_rounds`."""
    Hs, Ws = _u8_map(mask, "scene_split mask")
    r2 = 0 if float(r) == 0.0 else boundary_radius2(r)
    if not 1 <= int(max_rounds) <= 65536:
        raise ValueError(f"max_rounds must lie in [1, 65536], got {max_rounds}")
    if cls_map is not None:
        assert cls_map.dtype == torch.uint8 and cls_map.shape == mask.shape and cls_map.is_contiguous()
    if score is not None:
        assert score.dtype == torch.float32 and score.shape == mask.shape and score.is_contiguous()
    nbytes = L.lib().c3d_scene_split_ws_bytes(Hs, Ws, int(n_cls) if cls_map is not None else 1)
    if nbytes < 0 or int(max_objects) < 1:
        raise L.Change3DHipError(f"c3d_scene_split refuses a {Hs} x {Ws} scene with n_cls = {n_cls}, max_objects = "
                                 f"{max_objects} (code {nbytes if nbytes < 0 else -1})")
    dev = mask.device
    ws = _scene_ws(ws, nbytes, dev, "c3d_scene_split", Hs, Ws)
    labels = torch.empty((Hs, Ws), dtype=torch.int32, device=dev)
    table = torch.empty((int(max_objects), 8), dtype=torch.int32, device=dev)
    hist = torch.empty((int(max_objects), int(n_cls)), dtype=torch.int32, device=dev) if want_hist and cls_map is not None else None
    object_cls = torch.empty((Hs, Ws), dtype=torch.uint8, device=dev) if want_object_cls else None
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    _launch("c3d_scene_split", Hs * Ws * 80, L.lib().c3d_scene_split, _p(mask), _p(cls_map), _p(score), Hs, Ws, int(connectivity),
            int(min_area), int(n_cls), int(first_class), int(max_objects), r2, int(max_rounds), _p(labels), _p(table), _p(hist),
            _p(object_cls), _p(counts), _p(info), _p(ws), _stream())
    return labels, table, hist, object_cls, counts, info


def scene_regions_tile():
    """(th, tw) of the LDS tile of c3d_scene_regions' local phase; host only."""
    th, tw = C.c_int32(0), C.c_int32(0)
    L.check(L.lib().c3d_scene_regions_tile(C.byref(th), C.byref(tw)), "c3d_scene_regions_tile")
    return th.value, tw.value


def _region_score(score, key_map):
    if score is not None:
        assert score.dtype == torch.float32 and score.shape == key_map.shape and score.is_contiguous() and score.is_cuda


def scene_regions(key_map, score=None, connectivity=8, min_area=1, max_objects=65536, want_object_key=True, ws=None):
    """c3d_scene_regions on the u8 map `key_map` [Hs, Ws]: the connected components of equal nonzero key.  Returns `(labels i32
    [Hs, Ws], table i32 [max_objects, 8], None, object_key u8 [Hs, Ws] or None, counts i32 [2])`, the 5-tuple of
    `scene_objects`, all on the device; nothing is read back.  Column 5 of a table row is the region's key."""
    Hs, Ws = _u8_map(key_map, "scene_regions key map")
    _region_score(score, key_map)
    if int(max_objects) < 1:
        raise L.Change3DHipError(f"c3d_scene_regions refuses max_objects = {max_objects}")
    dev = key_map.device
    ws = _scene_ws(ws, L.lib().c3d_scene_regions_ws_bytes(Hs, Ws), dev, "c3d_scene_regions", Hs, Ws)
    labels = torch.empty((Hs, Ws), dtype=torch.int32, device=dev)
    table = torch.empty((int(max_objects), 8), dtype=torch.int32, device=dev)
    object_key = torch.empty((Hs, Ws), dtype=torch.uint8, device=dev) if want_object_key else None
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _launch("c3d_scene_regions", Hs * Ws * 40, L.lib().c3d_scene_regions, _p(key_map), _p(score), Hs, Ws, int(connectivity),
            int(min_area), int(max_objects), _p(labels), _p(table), _p(object_key), _p(counts), _p(ws), _stream())
    return labels, table, None, object_key, counts


def regions_sieve_plan(Hs, Ws, table_capacity=0):
    """c3d_regions_sieve_ws_bytes: (workspace bytes, table capacity); `table_capacity` 0 asks for the one that cannot overflow."""
    cap = C.c_int64(int(table_capacity))
    nbytes = L.lib().c3d_regions_sieve_ws_bytes(int(Hs), int(Ws), C.byref(cap))
    if nbytes < 0:
        raise L.Change3DHipError(f"c3d_regions_sieve refuses a {Hs} x {Ws} scene with a table of {table_capacity} slots (code {nbytes})")
    return int(nbytes), int(cap.value)


def regions_sieve(key_map, min_area, score=None, connectivity=8, max_rounds=8, max_objects=65536, table_capacity=0, ws=None):
    """c3d_regions_sieve on the u8 map `key_map` [Hs, Ws]: regions below `min_area` pixels are absorbed by the neighbour they
    share the longest border with, in rounds.  Returns `(labels, table, None, key_out u8 [Hs, Ws], counts, info i32 [8])`:
    `scene_regions(key_out)` and `info` = (status, rounds, regions moved, pixels changed, small regions left, regions of the
    input, most table entries of a round, 0), all on the device; nothing is read back.  A status with `SIEVE_ST_NOT_CONVERGED`
    asks for a larger `max_rounds`, one with `SIEVE_ST_TABLE_FULL` for a larger `table_capacity`."""
    Hs, Ws = _u8_map(key_map, "regions_sieve key map")
    _region_score(score, key_map)
    if not 1 <= int(min_area) <= 2 ** 20:
        raise ValueError(f"min_area must lie in [1, 2^20], got {min_area}")
    if not 1 <= int(max_rounds) <= 65536:
        raise ValueError(f"max_rounds must lie in [1, 65536], got {max_rounds}")
    if int(max_objects) < 1:
        raise L.Change3DHipError(f"c3d_regions_sieve refuses max_objects = {max_objects}")
    nbytes, cap = regions_sieve_plan(Hs, Ws, table_capacity)
    dev = key_map.device
    ws = _scene_ws(ws, nbytes, dev, "c3d_regions_sieve", Hs, Ws)
    key_out = torch.empty((Hs, Ws), dtype=torch.uint8, device=dev)
    labels = torch.empty((Hs, Ws), dtype=torch.int32, device=dev)
    table = torch.empty((int(max_objects), 8), dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    _launch("c3d_regions_sieve", Hs * Ws * 80, L.lib().c3d_regions_sieve, _p(key_map), _p(score), Hs, Ws, int(connectivity),
            int(min_area), int(max_rounds), int(max_objects), cap, _p(key_out), _p(labels), _p(table), _p(counts), _p(info), _p(ws),
            _stream())
    return labels, table, None, key_out, counts, info


def build_clip(pre, post, frames, clip, B, K, H, W):
    _launch("c3d_build_clip", clip.numel() * 8, L.lib().c3d_build_clip, _p(pre), _p(post), _p(frames), _p(clip), B, K, H, W,
            _stream())


# ------------------------------------------------------------------------------ caption decoder (change captioning)
def cap_embed_fwd(tokens, emb, pe, out, B, Lq, D, V, p, seed, dtype):
    _launch("c3d_cap_embed_fwd", out.numel() * _es(dtype), L.lib().c3d_cap_embed_fwd, _p(tokens), _p(emb), _p(pe), _p(out), B, Lq, D, V,
            float(p), int(seed), dtype, _stream())


def cap_embed_bwd(tokens, dout, demb, B, Lq, D, V, p, seed, dtype):
    _launch("c3d_cap_embed_bwd", dout.numel() * _es(dtype), L.lib().c3d_cap_embed_bwd, _p(tokens), _p(dout), _p(demb), B, Lq, D, V,
            float(p), int(seed), dtype, _stream())


def cap_dropout(x, y, rows, D, p, seed, dtype):
    _launch("c3d_cap_dropout", 2 * x.numel() * _es(dtype), L.lib().c3d_cap_dropout, _p(x), _p(y), rows, D, float(p), int(seed), dtype, _stream())


def cap_layernorm_fwd(x, a, ln, y, mr, rows, D, dtype):
    _launch("c3d_cap_layernorm_fwd", 3 * x.numel() * _es(dtype), L.lib().c3d_cap_layernorm_fwd, _p(x), _p(a), _p(ln.weight), _p(ln.bias), _p(y),
            _p(mr), rows, D, float(ln.eps), dtype, _stream())


def cap_layernorm_bwd(x, a, dy, ln, mr, dx, rows, D, dtype):
    _launch("c3d_cap_layernorm_bwd", 4 * x.numel() * _es(dtype), L.lib().c3d_cap_layernorm_bwd, _p(x), _p(a), _p(dy), _p(ln.weight), _p(mr), _p(dx),
            _p(grad_of(ln.weight)), _p(grad_of(ln.bias)), rows, D, dtype, _stream())


def cap_attn_fwd(q, k, v, ldq, ldk, ldv, o, ldo, P, B, H, Lq, Lk, hd, scale, causal, p, seed, dtype, q_off=0, k_off=0, v_off=0):
    es = _es(dtype)
    _launch("c3d_cap_attn_fwd", (q.numel() + k.numel() + o.numel()) * es, L.lib().c3d_cap_attn_fwd, q.data_ptr() + q_off * es,
            k.data_ptr() + k_off * es, v.data_ptr() + v_off * es, ldq, ldk, ldv, _p(o), ldo, _p(P), B, H, Lq, Lk, hd, float(scale),
            1 if causal else 0, float(p), int(seed), dtype, _stream())


def cap_attn_bwd(q, k, v, ldq, ldk, ldv, dout, ldo, P, dq, dk, dv, lddq, lddk, lddv, B, H, Lq, Lk, hd, scale, p, seed, dtype,
                 q_off=0, k_off=0, v_off=0, dq_off=0, dk_off=0, dv_off=0):
    es = _es(dtype)
    _launch("c3d_cap_attn_bwd", (q.numel() + k.numel() + dout.numel()) * 2 * es, L.lib().c3d_cap_attn_bwd, q.data_ptr() + q_off * es,
            k.data_ptr() + k_off * es, v.data_ptr() + v_off * es, ldq, ldk, ldv, _p(dout), ldo, _p(P), dq.data_ptr() + dq_off * es,
            dk.data_ptr() + dk_off * es, dv.data_ptr() + dv_off * es, lddq, lddk, lddv, B, H, Lq, Lk, hd, float(scale), float(p),
            int(seed), dtype, _stream())


def cap_ce_fwd(logits, caps, declen, acc2, lse, loss, B, Lq, V, ignore_index, dtype):
    _launch("c3d_cap_ce_fwd", logits.numel() * _es(dtype), L.lib().c3d_cap_ce_fwd, _p(logits), _p(caps), _p(declen), _p(acc2), _p(lse), _p(loss),
            B, Lq, V, ignore_index, dtype, _stream())


def cap_ce_bwd(logits, caps, declen, acc2, lse, dloss, dlogits, B, Lq, V, ignore_index, dtype):
    _launch("c3d_cap_ce_bwd", 2 * logits.numel() * _es(dtype), L.lib().c3d_cap_ce_bwd, _p(logits), _p(caps), _p(declen), _p(acc2), _p(lse), _p(dloss),
            _p(dlogits), B, Lq, V, ignore_index, dtype, _stream())


def clamp_(g, limit):
    _launch("c3d_clamp_", g.numel() * 8, L.lib().c3d_clamp_, _p(g), g.numel(), float(limit), _stream())


def cap_beam_plan(S, D, H, n_layer, V, beam, max_len, dtype, B=1):
    """c3d_cap_beam_plan: (workspace bytes, dynamic-LDS bytes) of a batched beam search, or None for a shape the kernel does
    not take (C3D_E_UNSUPPORTED).  Host only: callable without a GPU."""
    ws, lds = C.c_int64(0), C.c_int64(0)
    rc = L.lib().c3d_cap_beam_plan(S, D, H, n_layer, V, beam, max_len, dtype, B, C.byref(ws), C.byref(lds))
    if rc == -2:
        return None
    L.check(rc, "c3d_cap_beam_plan")
    return ws.value, lds.value


def cap_beam_search(dec, kv, B, S, start_id, end_id, beam, max_len, dtype, ws, comp_seq, comp_len, comp_score, meta, trace=None,
                    forced=None, logits_out=None):
    """c3d_cap_beam_search over B pairs: `dec` a CaptionDecoder (its parameters are read in place), `kv` the per-layer
    projected memory [S*B][2D] of model.caption_decoder.project_memory.  One launch, no synchronisation."""
    a = L.CapBeamArgs()
    D = dec.vocab_embedding.weight.shape[1]
    a.B, a.S, a.D, a.H, a.n_layer, a.V, a.beam, a.max_len = B, S, D, dec.n_head, len(dec.transformer.layers), dec.vocab_size, beam, max_len
    a.start_id, a.end_id, a.dtype = int(start_id), int(end_id), dtype
    a.ln_eps = float(dec.transformer.layers[0].norm1.eps)
    a.emb, a.pe = _p(dec.vocab_embedding.weight), _p(dec.position_encoding.pe)
    a.wdc_w, a.wdc_b = _p(dec.wdc.weight), _p(dec.wdc.bias)
    for i, (layer, kv2) in enumerate(zip(dec.transformer.layers, kv)):
        sa, ca, l = layer.self_attn, layer.multihead_attn2, a.layers[i]
        l.sa_in_w, l.sa_in_b, l.sa_out_w, l.sa_out_b = _p(sa.in_proj_weight), _p(sa.in_proj_bias), _p(sa.out_proj.weight), _p(sa.out_proj.bias)
        l.n1_g, l.n1_b, l.n2_g, l.n2_b = _p(layer.norm1.weight), _p(layer.norm1.bias), _p(layer.norm2.weight), _p(layer.norm2.bias)
        l.ca_q_w, l.ca_q_b = _p(ca.in_proj_weight), _p(ca.in_proj_bias)           # rows [:D] of the packed projection
        l.ca_out_w, l.ca_out_b, l.kv = _p(ca.out_proj.weight), _p(ca.out_proj.bias), _p(kv2)
    a.ws, a.comp_seq, a.comp_len, a.comp_score, a.meta = _p(ws), _p(comp_seq), _p(comp_len), _p(comp_score), _p(meta)
    a.trace, a.forced, a.logits_out = _p(trace), _p(forced), _p(logits_out)
    _launch("c3d_cap_beam_search", ws.numel() * ws.element_size(), L.lib().c3d_cap_beam_search, C.byref(a), _stream())


def cap_strip(raw, start_id, end_id, pad_id):
    """c3d_cap_strip: `raw` int32 [rows, L_in] on the device -> (tokens int32 [rows, 64], lengths int32 [rows]) without the three
    special ids, order kept (reference scripts/train_CC.py:336-343).  One launch, nothing read back."""
    assert raw.dtype == torch.int32 and raw.dim() == 2 and raw.is_contiguous()
    require_gpu(raw, "cap_strip input")
    rows, L_in = int(raw.shape[0]), int(raw.shape[1])
    out = torch.empty((rows, 64), dtype=torch.int32, device=raw.device)
    out_len = torch.empty(rows, dtype=torch.int32, device=raw.device)
    _launch("c3d_cap_strip", raw.numel() * 8, L.lib().c3d_cap_strip, _p(raw), rows, L_in, int(start_id), int(end_id), int(pad_id),
            _p(out), _p(out_len), _stream())
    return out, out_len


def cap_metrics_plan(N, R, Lr, ref_tokens=0, table_capacity=0):
    """c3d_cap_metrics_plan: (workspace bytes, table capacity), or None for a shape the kernels do not take
    (C3D_E_UNSUPPORTED).  Host only: callable without a GPU."""
    ws, cap = C.c_int64(0), C.c_int64(int(table_capacity))
    rc = L.lib().c3d_cap_metrics_plan(int(N), int(R), int(Lr), int(ref_tokens), C.byref(ws), C.byref(cap))
    if rc == -2:
        return None
    L.check(rc, "c3d_cap_metrics_plan")
    return ws.value, cap.value


def cap_metrics(hyp, hyp_len, refs, ref_len, sel=None, nochange=None, nochange_len=None, ref_tokens=0, table_capacity=0, ws=None):
    """c3d_cap_metrics on a corpus that lives on the device: hyp int32 [N, L], hyp_len int32 [N], refs int32 [N, R, L], ref_len
    int32 [N, R], optional sel int32 [M] and no-change rows int32 [K, L] / [K].  Returns a dict of device tensors -- stats i32
    [M, 10], lcs i32 [M, R], flags i32 [M], rouge / cider f64 [M], totals i64 [17], ws u8 (status and table), capacity --
    nothing is read back here: totals[16] is the status the caller must look at (include/change3d_hip.h).  `ws`: a u8 buffer of
    at least the plan's bytes to use instead of a fresh one (tests put a guard behind the table)."""
    for t in (hyp, hyp_len, refs, ref_len) + tuple(x for x in (sel, nochange, nochange_len) if x is not None):
        assert t.dtype == torch.int32 and t.is_contiguous()
        require_gpu(t, "cap_metrics input")
    N, Lr = int(hyp.shape[0]), int(hyp.shape[1])
    R = int(refs.shape[1])
    assert refs.shape == (N, R, Lr) and hyp_len.shape == (N,) and ref_len.shape == (N, R)
    M = N if sel is None else int(sel.numel())
    K = 0 if nochange is None else int(nochange.shape[0])
    assert K == 0 or (nochange.shape == (K, Lr) and nochange_len.shape == (K,))
    plan = cap_metrics_plan(N, R, Lr, ref_tokens, table_capacity)
    if plan is None or M < 1 or K > L.CAP_METRICS_MAX_NOCHANGE:
        raise L.Change3DHipError(f"c3d_cap_metrics refuses N = {N}, R = {R}, L = {Lr}, M = {M}, {K} no-change rows")
    nbytes, cap = plan
    dev = hyp.device
    assert ws is None or (ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_contiguous() and ws.data_ptr() % 256 == 0)
    out = {"ws": torch.empty(nbytes, dtype=torch.uint8, device=dev) if ws is None else ws, "capacity": cap,
           "stats": torch.empty((M, 10), dtype=torch.int32, device=dev), "lcs": torch.empty((M, R), dtype=torch.int32, device=dev),
           "flags": torch.empty(M, dtype=torch.int32, device=dev), "rouge": torch.empty(M, dtype=torch.float64, device=dev),
           "cider": torch.empty(M, dtype=torch.float64, device=dev),
           "totals": torch.empty(L.CAP_TOTALS, dtype=torch.int64, device=dev)}
    a = L.CapMetricsArgs()
    a.N, a.R, a.L, a.M, a.n_nochange, a.table_capacity = N, R, Lr, M, K, cap
    a.hyp, a.hyp_len, a.refs, a.ref_len, a.sel = _p(hyp), _p(hyp_len), _p(refs), _p(ref_len), _p(sel)
    a.nochange, a.nochange_len, a.ws = _p(nochange) if K else None, _p(nochange_len) if K else None, _p(out["ws"])
    a.stats, a.lcs, a.flags, a.rouge, a.cider, a.totals = (_p(out[k]) for k in ("stats", "lcs", "flags", "rouge", "cider", "totals"))
    _launch("c3d_cap_metrics", nbytes + (N * (R + 1) * Lr) * 4, L.lib().c3d_cap_metrics, C.byref(a), _stream())
    return out


def linear_fwd(x, weight, bias, y, M, K, N, dtype):
    """y[M][Np] = x[M][Kp] @ weight[N][K]^T + bias (nn.Linear / in_proj slices)."""
    pw_gemm(x, weight, y, M=M, K=K, N=N, w_sn=weight.stride(0), w_sk=1, dtype=dtype, bias=bias)


def linear_bwd(x, weight, dy, dx, gw, gb, M, K, N, dtype, accumulate_dx=None):
    """dx = dy @ weight (written, or added to `accumulate_dx`), gw += dy^T x, gb += colsum(dy)."""
    if dx is not None:
        pw_gemm(dy, weight, dx, M=M, K=N, N=K, w_sn=1, w_sk=weight.stride(0), dtype=dtype,
                epi_mode=EPI_ADD if accumulate_dx is not None else EPI_STORE, e1=accumulate_dx, res_mode=0)
    pw_wgrad(dy, x, gw, M=M, K=K, N=N, dw_sn=gw.stride(0), dw_sk=1, dtype=dtype)
    if gb is not None:
        col_sum(dy, gb, M, N, dtype)
