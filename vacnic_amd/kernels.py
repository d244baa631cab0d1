"""Thin, non-autograd wrappers: torch tensors in, raw device pointers through the C-ABI.

PyTorch here is plumbing only (device memory + the current HIP stream); every arithmetic op on the
path is a hand-written gfx950 kernel in libvacnic_hip.so.  All wrappers launch on
`torch.cuda.current_stream()` so they are hipGraph-capturable, and all fail loudly on CPU tensors.
"""
import collections
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import call, call_struct

ACT = {None: 0, "none": 0, "gelu": 1, "tanh": 2, "quick_gelu": 3}
BF16 = torch.bfloat16


_HAVE_GPU = None
DETERMINISTIC = False     # ops.set_deterministic(): every fp32 sum whose order depended on scheduling takes a fixed-order kernel instead
                          # (vacnic_*_ordered, include/vacnic_hip.h).  Read at launch time, so a launch plan replays the mode it was
                          # recorded in.
_OVERRIDE = None          # raw hipStream_t set by launch_on(): lets ops issue a few launches on a side stream without
                          # paying for torch.cuda.stream()'s context switch (~10 us of host time per use)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """Raw hipStream_t of torch's current stream on the current device (the ~0.3 us C query, not the Python
    `torch.cuda.current_stream()` object that costs ~8 us per call and was 10 ms of host time per training step)."""
    global _HAVE_GPU
    if _HAVE_GPU is None:
        _HAVE_GPU = torch.cuda.is_available()
    if not _HAVE_GPU:
        raise RuntimeError("vacnic_amd kernels need an MI355X (HIP device): there is no CPU fallback")
    if _OVERRIDE is not None:
        return _OVERRIDE
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class launch_on:
    """with launch_on(raw_stream): every vacnic kernel wrapper inside launches on that HIP stream (torch's notion of the
    current stream is untouched, so allocations stay on the caller's stream — the caller owns the ordering/lifetime).

    fence=True (default): the side stream first waits for everything enqueued on torch's current stream so far.  torch's
    allocator believes every block lives on the current stream and hands a freed block out again at once; a kernel launched on
    the side stream into such a block must not overtake the compute-stream kernels that were still using it.

    Lifetime: every tensor a kernel wrapper is handed inside the section goes onto the side-stream keep-list (_p) and stays
    referenced until the compute stream has joined that stream (streams.join_all).  The list has no other
    writer: call sites keep nothing by hand, so a wrapper that may run on a side stream passes every
    tensor of the call through _p."""

    def __init__(self, raw, fence=True):
        self.raw, self.fence = raw, fence

    def __enter__(self):
        global _OVERRIDE
        self.prev = _OVERRIDE
        if self.fence and self.raw is not None and self.raw != self.prev:
            cur = _raw_stream(torch.cuda.current_device()) if _raw_stream is not None else torch.cuda.current_stream().cuda_stream
            if cur != self.raw:
                call("vacnic_stream_fence", cur, self.raw)
        _OVERRIDE = self.raw

    def __exit__(self, *exc):
        global _OVERRIDE
        _OVERRIDE = self.prev
        return False


_KEEP = None            # streams.py's keep-list: tensors handed to a kernel on a side stream stay referenced until the join


def _p(t):
    """device address of `t` for the C-ABI; inside a launch_on section it also puts `t` on the keep-list (see launch_on)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("vacnic_amd kernels need CUDA/HIP tensors (there is no CPU fallback)")
    if _OVERRIDE is not None and _KEEP is not None:
        # launched on a side stream while torch's allocator believes everything lives on the current stream: the block must not be
        # handed out again before the compute stream has joined that side stream (streams.join_all drops the references)
        _KEEP.append(t)
    return t.data_ptr()


# ------------------------------------------------------------------------------------- communication
def comm_load():
    """resolve librccl for the comm entry points (the copy torch ships and has already loaded, else the system one)."""
    import os
    p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    call("vacnic_comm_load", p.encode() if os.path.exists(p) else None)


def comm_unique_id():
    buf = _lib.C.create_string_buffer(128)
    call("vacnic_comm_unique_id", buf)
    return buf.raw


def comm_init(id128, rank, world):
    h = int(_lib.lib.vacnic_comm_init(_lib.C.c_char_p(id128), rank, world))
    if h < 0:
        _lib.check(4)
    return h


def allreduce_bucket(comm, t):
    """in-place SUM all-reduce of a contiguous fp32 / bf16 tensor over the RCCL communicator, on the launch stream."""
    assert t.is_contiguous() and t.dtype in (torch.float32, BF16)
    call("vacnic_allreduce_bucket", comm, _p(t), t.numel(), 0 if t.dtype == torch.float32 else 1, _stream())


def comm_broadcast(comm, t, root=0):
    assert t.is_contiguous() and t.dtype in (torch.float32, BF16)
    call("vacnic_comm_broadcast", comm, _p(t), t.numel(), 0 if t.dtype == torch.float32 else 1, root, _stream())


def event_record(slot, stream=None):
    call("vacnic_event_record", slot, stream if stream is not None else _stream())


def event_wait(slot, stream=None):
    call("vacnic_event_wait", slot, stream if stream is not None else _stream())


def recording():
    """a launch plan is being recorded by this process (vacnic_plan_begin .. vacnic_plan_end)."""
    return int(_lib.lib.vacnic_plan_mark()) >= 0


def fence(src_raw, dst_raw):
    """stream `dst` waits for everything enqueued on stream `src` so far (raw hipStream_t handles) — the recordable form of
    event.record(src); dst.wait_event(event) (vacnic_stream_fence): cross-stream edges are part of a launch plan."""
    if src_raw != dst_raw:
        call("vacnic_stream_fence", src_raw, dst_raw)


def _row_stride(t):
    """t is [..., rows, cols] with unit inner stride and uniformly strided rows when flattened."""
    assert t.stride(-1) == 1, "inner dimension must be contiguous"
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


# ------------------------------------------------------------------------------------------------ GEMM
GEMM_LOG = None           # tools/autotune_gemm.py sets this to a list to record call signatures
GEMM_TUNED = {}           # "xk,wk,M,N,K,out_mode,has_preact" -> [tile_hint, split_k, ...] measured winners (gemm_tuned.json)


def _load_tuned():
    import json, os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tuned.json")
    if os.path.exists(path) and os.environ.get("VACNIC_GEMM_TUNED", "1") != "0":
        with open(path) as f:
            GEMM_TUNED.update(json.load(f))


_load_tuned()


_FIX = {}                 # launch stream -> [workspace (uint8), counters (int32, all zero between launches)]
_FIX_CAPTURE = {}         # the same for launches recorded by a hipGraph capture on that stream (buffers from the graph's private pool)
_CAPTURE_SCOPE = 0        # owner of the graph being captured (capture_scope); 0: graphs that replay in order on one stream
_FIX_OLD = []             # outgrown workspaces: kernels already enqueued may still use them


@contextlib.contextmanager
def capture_scope(tag):
    """fix-up buffers of launches captured inside this block are private to `tag` (any hashable: the object that owns the graphs).
    torch captures every graph on ONE capture stream, so the per-stream table alone would hand the image-tower graph, the encoder
    graph and a decode session's graphs the same workspace and counters — fine while graphs replay one after the other on one stream,
    wrong once generate.CaptionPipeline replays them on several streams at once."""
    global _CAPTURE_SCOPE
    prev, _CAPTURE_SCOPE = _CAPTURE_SCOPE, tag
    try:
        yield
    finally:
        _CAPTURE_SCOPE = prev


def _fix_buffers(stream, M, N, split_k):
    """split-K fix-up buffers of the launch stream: launches on ONE stream run in order, so they share a workspace that only
    grows (persistent: the same addresses at every replay of a launch plan), and the arrival counters, which every launch leaves
    zeroed.  Kept out of torch's per-step allocations on purpose.  The counters of a new buffer are cleared ON THE LAUNCH STREAM
    (vacnic_zero_bytes: ordered before the GEMM whatever stream torch considers current; a fill kernel inside a stream capture).
    Launches recorded by a hipGraph capture get buffers of their own (allocated from the graph's pool): a captured launch and an
    eager one must never share counters; graphs captured in one scope (capture_scope) replay in order on one stream."""
    need = int(_lib.lib.vacnic_gemm_workspace_bytes(M, N, split_k))
    ncnt = int(_lib.lib.vacnic_gemm_counters(M, N))
    capturing = torch.cuda.is_current_stream_capturing()
    table = _FIX_CAPTURE if capturing else _FIX
    # graphs that may replay CONCURRENTLY (generate.GraphedCall: image tower / encoder) never share buffers
    key = (stream, _CAPTURE_SCOPE) if capturing else stream
    ent = table.get(key)
    if ent is None or ent[0].numel() < need or ent[1].numel() < ncnt:
        floor = 0 if capturing else 64 << 20
        ws = torch.empty(max(need, ent[0].numel() if ent else 0, floor), device="cuda", dtype=torch.uint8)
        cnt = torch.empty(max(ncnt, ent[1].numel() if ent else 0, 4096), device="cuda", dtype=torch.int32)
        call("vacnic_zero_bytes", cnt.data_ptr(), cnt.numel() * 4, stream)
        if ent is not None:
            _FIX_OLD.append(ent)
        ent = table[key] = [ws, cnt]
    return ent


def gemm(x, w, M, N, K, *, bias=None, out=None, ldx=None, ldw=None, ldo=None, x_kstrided=False, w_kstrided=False,
         act=None, out_mode=0, split_k=1, alpha=1.0, preact=None, dact_src=None, residual=None, tile_hint=0, xsum=None, fixup=False,
         drop=None):
    """out[m][n] = epi(alpha * sum_k X(m,k) W(n,k) + bias[n]) — see include/vacnic_hip.h.
    tile_hint 0: measured winner for this exact shape if gemm_tuned.json has one, else the C-side cost model; -1: cost model.
    fixup: split_k > 1 through the ordered fix-up (no atomics, bitwise reproducible, any out_mode) instead of fp32 atomics.
    drop: (p, seed, seed_dev tensor or None) — activation dropout in the epilogue (after act / act'); see can_fuse_dropout."""
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=BF16 if out_mode == 0 else torch.float32)
    ldx = ldx if ldx is not None else (M if x_kstrided else K)
    ldw = ldw if ldw is not None else (N if w_kstrided else K)
    ldo = ldo if ldo is not None else N
    if GEMM_LOG is not None:
        GEMM_LOG.append((int(x_kstrided), int(w_kstrided), M, N, K, ldx, ldw, ldo, out_mode, split_k, bias is not None, act,
                         preact is not None, dact_src is not None, residual is not None))
    if tile_hint == 0 and GEMM_TUNED:
        t = GEMM_TUNED.get(f"{int(x_kstrided)},{int(w_kstrided)},{M},{N},{K},{out_mode},{int(preact is not None)}")
        if t is not None and len(t) > 4 and t[4]:
            # measured winner = K slices through the ordered fix-up (long reductions into a small output: too few tiles to fill
            # 256 CUs unsplit, and a bf16 / activation / residual epilogue cannot meet in atomics)
            if split_k == 1:
                tile_hint, split_k, fixup = t[0], t[1], True
        elif t is not None:
            tile_hint = t[0] or -1
            if out_mode == 2:
                split_k = t[1]
    if tile_hint < 0:
        tile_hint = 0
    if DETERMINISTIC and out_mode == 2 and split_k > 1:
        fixup = True                          # (fp32 atomics into `out` otherwise: the order of the K slices would be the scheduler's)
    st = _stream()
    ws = wsb = cnt = cntn = None
    if fixup and split_k > 1:
        wbuf, cbuf = _fix_buffers(st, M, N, split_k)
        ws, wsb, cnt, cntn = wbuf.data_ptr(), wbuf.numel(), cbuf.data_ptr(), cbuf.numel()
    call_struct("vacnic_gemm_bf16", stream=st, x=_p(x), w=_p(w), bias=_p(bias), out=_p(out), preact=_p(preact),
                dact_src=_p(dact_src), residual=_p(residual), xsum=_p(xsum), M=M, N=N, K=K, ldx=ldx, ldw=ldw, ldo=ldo,
                x_kstrided=int(x_kstrided), w_kstrided=int(w_kstrided), act=ACT[act], out_mode=out_mode,
                split_k=split_k, alpha=alpha, tile_hint=tile_hint, workspace=ws, workspace_bytes=wsb or 0, counters=cnt,
                counters_len=cntn or 0, drop_p=float(drop[0]) if drop else 0.0, drop_seed=int(drop[1]) if drop else 0,
                drop_seed_dev=_p(drop[2]) if drop else None)
    return out


def gemm_plan(M, N, K, *, x_kstrided=False, w_kstrided=False, ldx=None, ldw=None, ldo=None, act=None, out_mode=0, split_k=1, alpha=1.0,
              bias=False, preact=False, dact_src=False, residual=False, xsum=False, tile_hint=-1, fixup=False, drop_p=0.0, ptrs=None):
    """what gemm() would launch for this call (vacnic_gemm_plan: the launch path's own decision code, no GPU needed): a list with
    one dict per launch, keys rows / tile_hint / k_slices / fixup / epilogue (a name from _lib.EPI_NAMES).  Operands are flags
    (any aligned address stands in for a present one) unless `ptrs` gives addresses by name; tile_hint as in gemm(), except that
    0 is NOT looked up in gemm_tuned.json here.  Raises what gemm() would raise."""
    fake = 1 << 20
    ptr = {"x": fake, "w": fake, "out": fake, "bias": fake if bias else None, "preact": fake if preact else None,
           "dact_src": fake if dact_src else None, "residual": fake if residual else None, "xsum": fake if xsum else None}
    ptr.update(ptrs or {})
    ws = wsb = cnt = cntn = None
    if fixup and split_k > 1:
        ws, cnt = fake, fake
        wsb, cntn = int(_lib.lib.vacnic_gemm_workspace_bytes(M, N, split_k)), int(_lib.lib.vacnic_gemm_counters(M, N))
    a = _lib.GemmArgs(M=M, N=N, K=K, ldx=ldx if ldx is not None else (M if x_kstrided else K),
                      ldw=ldw if ldw is not None else (N if w_kstrided else K), ldo=ldo if ldo is not None else N,
                      x_kstrided=int(x_kstrided), w_kstrided=int(w_kstrided), act=ACT[act], out_mode=out_mode, split_k=split_k,
                      alpha=alpha, tile_hint=max(tile_hint, 0), workspace=ws, workspace_bytes=wsb or 0, counters=cnt,
                      counters_len=cntn or 0, drop_p=float(drop_p), drop_seed=0, drop_seed_dev=None, **ptr)
    out = _lib.GemmPlanOut()
    _lib.check(_lib.lib.vacnic_gemm_plan(ctypes.byref(a), ctypes.byref(out)))
    return [dict(rows=int(out.rows[i]), tile_hint=int(out.tile_hint[i]), k_slices=int(out.k_slices[i]), fixup=bool(out.fixup[i]),
                 epilogue=_lib.EPI_NAMES[out.epilogue[i]]) for i in range(out.nlaunch)]


def can_fuse_dropout(N, ldo=None):
    """the GEMM epilogue can apply activation dropout to a contiguous [M, N] bf16 output with N % 16 == 0."""
    return N % 16 == 0 and (ldo is None or ldo == N)


def gemv_ln(x, residual, gamma, beta, w, M, N, Kd, *, bias=None, out=None, ln_out=None, ldw=None, ldo=None, act=None, out_mode=0, eps=1e-5):
    """out = epi(LayerNorm(x + residual) . w^T + bias) for M <= 8 rows; ln_out (optional) receives the normalised rows."""
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=BF16 if out_mode == 0 else torch.float32)
    call_struct("vacnic_gemv_ln_bf16", stream=_stream(), x=_p(x), residual=_p(residual), gamma=_p(gamma), beta=_p(beta), ln_out=_p(ln_out),
                w=_p(w), bias=_p(bias), out=_p(out), M=M, N=N, K=Kd, ldw=ldw if ldw is not None else Kd, ldo=ldo if ldo is not None else N,
                act=ACT[act], out_mode=out_mode, eps=eps)
    return out


def wgrad_split(M_red, n_tiles):
    """split-K factor for a weight gradient whose reduction runs over M_red rows: aim at >= 512 workgroups."""
    s = 1
    while n_tiles * s < 512 and M_red // (s * 2) >= 512 and s < 16:
        s *= 2
    return s


def wgrad_group(jobs):
    """jobs: list of (dy2d [M,N] bf16, x2d [M,K] bf16, dw [N,K] f32 view, dbias [N] f32 or None): dw += dy^T x, dbias += colsum(dy)
    for all of them in one launch per 16 output blocks of 1024 x 1024 — no split-K, no atomics on dw (vacnic_wgrad_group)."""
    arr = (_lib.WgradJob * len(jobs))()
    for j, (dy, x, dw, db) in enumerate(jobs):
        M, N = dy.shape
        Kd = x.shape[1]
        assert x.shape[0] == M and tuple(dw.shape) == (N, Kd) and dy.stride(1) == 1 and x.stride(1) == 1 and dw.stride(1) == 1
        a = arr[j]
        a.dy, a.x, a.dw, a.dbias = _p(dy), _p(x), _p(dw), _p(db)
        a.M, a.N, a.K, a.lddy, a.ldx, a.lddw = M, N, Kd, dy.stride(0), x.stride(0), dw.stride(0)
    call("vacnic_wgrad_group", arr, len(jobs), _stream())


# ------------------------------------------------------------------------------------------- attention
def attn_fwd(q, k, v, B, H, Tq, Tk, key_mask=None, causal=False, scale=0.125, need_lse=True, p_drop=0.0, seed=0, seed_dev=None):
    """q/k/v: [B, T, >=H*64] views (unit inner stride); returns out [B,Tq,H*64] bf16 and lse [B,H,Tq]."""
    out = torch.empty((B, Tq, H * 64), device=q.device, dtype=BF16)
    lse = torch.empty((B, H, Tq), device=q.device, dtype=torch.float32) if need_lse else None
    call_struct("vacnic_attn_fwd", stream=_stream(), q=_p(q), k=_p(k), v=_p(v), out=_p(out), lse=_p(lse),
                key_mask=_p(key_mask), B=B, H=H, Tq=Tq, Tk=Tk, ldq=q.stride(1), ldk=k.stride(1), ldv=v.stride(1),
                ldo=out.stride(1), bsq=q.stride(0), bsk=k.stride(0), bsv=v.stride(0), bso=out.stride(0),
                causal=int(causal), scale=scale, p_drop=p_drop, seed=seed, seed_dev=_p(seed_dev))
    return out, lse


def attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, Tq, Tk, key_mask=None, causal=False, scale=0.125, p_drop=0.0, seed=0, seed_dev=None):
    delta = torch.empty((B, H, Tq), device=q.device, dtype=torch.float32)
    assert dout.stride() == out.stride()
    call_struct("vacnic_attn_bwd", stream=_stream(), q=_p(q), k=_p(k), v=_p(v), out=_p(out), dout=_p(dout), lse=_p(lse),
                delta=_p(delta), dq=_p(dq), dk=_p(dk), dv=_p(dv), key_mask=_p(key_mask), B=B, H=H, Tq=Tq, Tk=Tk,
                ldq=q.stride(1), ldk=k.stride(1), ldv=v.stride(1), ldo=out.stride(1),
                bsq=q.stride(0), bsk=k.stride(0), bsv=v.stride(0), bso=out.stride(0),
                lddq=dq.stride(1), lddk=dk.stride(1), lddv=dv.stride(1),
                bsdq=dq.stride(0), bsdk=dk.stride(0), bsdv=dv.stride(0), causal=int(causal), scale=scale, p_drop=p_drop, seed=seed,
                seed_dev=_p(seed_dev))


def attn_probs(q, k, B, H, Tq, Tk, key_mask=None, causal=False, scale=0.125):
    """softmax(scale q k^T + masks) as fp32 [B, H, Tq, Tk] (MFULL:509-544, before dropout) from the q / k views attn_fwd takes:
    masked keys and the causal triangle exactly 0, a fully masked row uniform 1/Tk.  Plain tensor, no autograd graph."""
    for name, t, T in (("q", q, Tq), ("k", k, Tk)):
        if t.dtype != BF16 or t.dim() != 3 or t.stride(2) != 1 or t.shape[0] != B or t.shape[1] != T:
            raise ValueError(f"attn_probs: {name} must be a bf16 [B={B}, T={T}, >= H*64] view with unit inner stride, got "
                             f"{t.dtype} {tuple(t.shape)} strides {t.stride()}")
    if key_mask is not None and (key_mask.dtype != torch.uint8 or tuple(key_mask.shape) != (B, Tk) or not key_mask.is_contiguous()):
        raise ValueError(f"attn_probs: key_mask must be a contiguous uint8 [B={B}, Tk={Tk}] tensor, got {key_mask.dtype} {tuple(key_mask.shape)}")
    out = torch.empty((B, H, Tq, Tk), device=q.device, dtype=torch.float32)
    call_struct("vacnic_attn_probs", stream=_stream(), q=_p(q), k=_p(k), out=_p(out), key_mask=_p(key_mask), B=B, H=H, Tq=Tq, Tk=Tk,
                ldq=q.stride(1), ldk=k.stride(1), bsq=q.stride(0), bsk=k.stride(0), causal=int(causal), scale=scale)
    return out


# -------------------------------------------------------------------------------------------- LN family
def add_ln_fwd(x, residual, gamma, beta, eps=1e-5, p_drop=0.0, seed=0, need_stats=True, seed_dev=None):
    D = x.shape[-1]
    R = x.numel() // D if D else 0          # D = 0: no rows; the entry point refuses the empty operands
    out = torch.empty_like(x)
    mean = torch.empty(R, device=x.device, dtype=torch.float32) if need_stats else None
    rstd = torch.empty(R, device=x.device, dtype=torch.float32) if need_stats else None
    call_struct("vacnic_add_ln_fwd", stream=_stream(), x=_p(x), residual=_p(residual), gamma=_p(gamma), beta=_p(beta),
                out=_p(out), mean=_p(mean), rstd=_p(rstd), R=R, D=D, eps=eps, p_drop=p_drop, seed=seed, seed_dev=_p(seed_dev))
    return out, mean, rstd


def add_ln_bwd(dout, x, residual, gamma, mean, rstd, dgamma, dbeta, p_drop=0.0, seed=0, need_dres=True, seed_dev=None, fold_on=None):
    """fold_on: raw stream for the dgamma / dbeta fold of the two-stage reduction (None: in the call, on the launch stream).  The
    fold is a 5 us kernel nobody in the backward chain waits for; the caller orders `fold_on` behind this launch's stream."""
    D = x.shape[-1]
    R = x.numel() // D if D else 0          # D = 0: no rows; the entry point refuses the empty operands
    dx = torch.empty_like(x)
    if residual is None or not need_dres:
        dres = None
    elif p_drop > 0.0:
        dres = torch.empty_like(x)
    else:
        dres = None            # identical to dx: caller reuses dx
    part, prow = None, 0
    if DETERMINISTIC and dgamma is not None and dbeta is not None and R >= 1:
        # every R through the per-block column sums (the kernel's block-to-row map depends on R alone) and the ordered fold: no atomic
        # anywhere.  The fold stays off the backward chain when the caller names a stream for it; `part` (like dgamma / dbeta) is then
        # on the side-stream keep-list until the compute stream has joined that stream (_p inside launch_on).
        prow = min(1024, (R + 3) // 4)
        part = torch.empty((prow, 2, D), device=x.device, dtype=torch.float32)
        call_struct("vacnic_add_ln_bwd", stream=_stream(), dout=_p(dout), x=_p(x), residual=_p(residual), gamma=_p(gamma),
                    mean=_p(mean), rstd=_p(rstd), dresidual=_p(dres), dx=_p(dx), dgamma=_p(dgamma), dbeta=_p(dbeta),
                    R=R, D=D, p_drop=p_drop, seed=seed, seed_dev=_p(seed_dev), partials=_p(part), partial_rows=prow, defer_fold=1,
                    partials_any=1)
        if fold_on is not None and fold_on != _stream():
            fence(_stream(), fold_on)
            with launch_on(fold_on, fence=False):
                fold_ordered(part, dgamma, dbeta, prow, D, ld=2 * D)
        else:
            fold_ordered(part, dgamma, dbeta, prow, D, ld=2 * D)
        return dx, (dres if dres is not None else dx)
    if dgamma is not None and R >= 256:         # two-stage dgamma / dbeta reduction (below 256 rows: per-column atomics)
        prow = min(1024, (R + 3) // 4)
        part = torch.empty((prow, 2, D), device=x.device, dtype=torch.float32)     # scratch of the two-stage dgamma/dbeta fold
    defer = fold_on is not None and part is not None and fold_on != _stream()
    call_struct("vacnic_add_ln_bwd", stream=_stream(), dout=_p(dout), x=_p(x), residual=_p(residual), gamma=_p(gamma),
                mean=_p(mean), rstd=_p(rstd), dresidual=_p(dres), dx=_p(dx), dgamma=_p(dgamma), dbeta=_p(dbeta),
                R=R, D=D, p_drop=p_drop, seed=seed, seed_dev=_p(seed_dev), partials=_p(part), partial_rows=prow, defer_fold=int(defer))
    if defer:
        fence(_stream(), fold_on)
        with launch_on(fold_on, fence=False):
            call("vacnic_ln_partial_fold", _p(part), _p(dgamma), _p(dbeta), prow, D, _stream())
    return dx, (dres if dres is not None else dx)


def dropout_(x, p_drop, seed, seed_dev=None):
    """in-place inverted dropout of a contiguous bf16 tensor (activation dropout; the same call on the gradient is its backward)."""
    assert x.is_contiguous() and x.dtype == BF16
    call("vacnic_dropout_bf16", _p(x), _p(x), x.numel(), float(p_drop), int(seed), _p(seed_dev), _stream())
    return x


def embed_ln_fwd(ids, embed16, pos16, gamma, beta, embed_scale=1.0, pos_offset=2, eps=1e-5, p_drop=0.0, seed=0, seed_dev=None):
    B, T = ids.shape
    V, D = embed16.shape
    out = torch.empty((B, T, D), device=ids.device, dtype=BF16)
    mean = torch.empty(B * T, device=ids.device, dtype=torch.float32)
    rstd = torch.empty(B * T, device=ids.device, dtype=torch.float32)
    call_struct("vacnic_embed_ln_fwd", stream=_stream(), ids=_p(ids), embed=_p(embed16), pos=_p(pos16), gamma=_p(gamma),
                beta=_p(beta), out=_p(out), mean=_p(mean), rstd=_p(rstd), B=B, T=T, D=D, V=V, pos_offset=pos_offset,
                embed_scale=embed_scale, eps=eps, p_drop=p_drop, seed=seed, seed_dev=_p(seed_dev))
    return out, mean, rstd


def embed_ln_bwd(ids, embed16, pos16, dout, gamma, mean, rstd, dembed, dpos, dgamma, dbeta, embed_scale=1.0,
                 pos_offset=2, padding_idx=1, p_drop=0.0, seed=0, seed_dev=None):
    B, T = ids.shape
    V, D = embed16.shape
    if DETERMINISTIC and B * T > 0:
        # no float atomics: dh rows to an fp32 scratch, then the ordered scatter (ascending row per id / position) and the ordered fold
        prow = min(1024, (B * T + 3) // 4)
        dh = torch.empty((B * T, D), device=ids.device, dtype=torch.float32)
        part = torch.empty((prow, 2, D), device=ids.device, dtype=torch.float32)
        st = _lib.EmbedLnBwdArgs(ids=_p(ids), embed=_p(embed16), pos=_p(pos16), dout=_p(dout), gamma=_p(gamma), mean=_p(mean),
                                 rstd=_p(rstd), dembed=_p(dembed), dpos=_p(dpos), dgamma=_p(dgamma), dbeta=_p(dbeta), B=B, T=T, D=D, V=V,
                                 pos_offset=pos_offset, embed_scale=embed_scale, padding_idx=padding_idx, p_drop=p_drop, seed=seed,
                                 seed_dev=_p(seed_dev))
        call("vacnic_embed_ln_bwd_ordered", ctypes.byref(st), _p(dh), _p(part), prow, _stream())
        return
    call_struct("vacnic_embed_ln_bwd", stream=_stream(), ids=_p(ids), embed=_p(embed16), pos=_p(pos16), dout=_p(dout),
                gamma=_p(gamma), mean=_p(mean), rstd=_p(rstd), dembed=_p(dembed), dpos=_p(dpos), dgamma=_p(dgamma),
                dbeta=_p(dbeta), B=B, T=T, D=D, V=V, pos_offset=pos_offset, embed_scale=embed_scale,
                padding_idx=padding_idx, p_drop=p_drop, seed=seed, seed_dev=_p(seed_dev))


def name_embed_mean(ids3d, embed16, pos16, gamma, beta, embed_scale=1.0, pos_offset=2, eps=1e-5):
    B, Nn, Ln = ids3d.shape
    V, D = embed16.shape
    out = torch.empty((B, Nn, D), device=ids3d.device, dtype=torch.float32)
    call_struct("vacnic_name_embed_mean", stream=_stream(), ids=_p(ids3d), embed=_p(embed16), pos=_p(pos16),
                gamma=_p(gamma), beta=_p(beta), out=_p(out), B=B, Nn=Nn, Ln=Ln, D=D, V=V, pos_offset=pos_offset,
                embed_scale=embed_scale, eps=eps)
    return out


# ------------------------------------------------------------------------------------------------ losses
def ce_fwd(logits, targets, V, ignore_index=1, label_smoothing=0.0):
    """label_smoothing: torch's CrossEntropyLoss(label_smoothing=) over the V real columns; 0.0 launches the plain kernels."""
    R, ldl = logits.shape[0], logits.stride(0)
    dev = logits.device
    row_lse = torch.empty(R, device=dev, dtype=torch.float32)
    if DETERMINISTIC:
        return _ce_fwd_ordered(logits, targets, V, ignore_index, label_smoothing, row_lse)[:2]
    acc = torch.zeros(2, device=dev, dtype=torch.float32)       # {loss_sum, count}
    call_struct("vacnic_ce_fwd", stream=_stream(), logits=_p(logits), targets=_p(targets), row_lse=_p(row_lse),
                row_loss=None, loss_sum=acc.data_ptr(), count=acc.data_ptr() + 4, dlogits=None, grad_out=None,
                grad_scale=1.0, R=R, V=V, ldl=ldl, ldd=ldl, ignore_index=ignore_index,
                logits_f32=int(logits.dtype == torch.float32), label_smoothing=label_smoothing)
    return row_lse, acc


def _ce_fwd_ordered(logits, targets, V, ignore_index, label_smoothing, row_lse):
    """ce_fwd in the deterministic mode -> (row_lse, acc, row_loss): the same kernel writes its per-row loss terms (an exact 0 on
    ignored rows) and adds its loss atomics into a word nobody reads; loss_sum is the ordered sum of the terms.  `count`, a sum of
    1.0s, is exact in any order and stays the kernel's."""
    R, ldl = logits.shape[0], logits.stride(0)
    dev = logits.device
    acc = zero_(torch.empty(4, device=dev, dtype=torch.float32))          # {loss_sum, count, the kernel's own atomic loss sum, -}
    row_loss = torch.empty(R, device=dev, dtype=torch.float32)
    call_struct("vacnic_ce_fwd", stream=_stream(), logits=_p(logits), targets=_p(targets), row_lse=_p(row_lse),
                row_loss=_p(row_loss), loss_sum=acc.data_ptr() + 8, count=acc.data_ptr() + 4, dlogits=None, grad_out=None,
                grad_scale=1.0, R=R, V=V, ldl=ldl, ldd=ldl, ignore_index=ignore_index,
                logits_f32=int(logits.dtype == torch.float32), label_smoothing=label_smoothing)
    sum_ordered(row_loss, acc)
    return row_lse, acc, row_loss


def sum_ordered(src, dst):
    """dst[0] = sum of the fp32 vector src in the documented fixed order (vacnic_sum_ordered)."""
    assert src.dtype == torch.float32 and src.is_contiguous() and dst.dtype == torch.float32
    call("vacnic_sum_ordered", _p(src), src.numel(), _p(dst), _stream())


def fold_ordered(partials, dst, dst2, NB, cols, ld=None):
    """dst[c] += sum_b partials[b][c] (and dst2[c] += sum_b partials[b][cols + c]) in the documented fixed order, one writer per
    element (vacnic_fold_ordered).  partials: fp32, rows `ld` floats apart (default: cols, or 2 cols with dst2)."""
    if ld is None:
        ld = cols * (2 if dst2 is not None else 1)
    call("vacnic_fold_ordered", _p(partials), ld, _p(dst), _p(dst2), NB, cols, _stream())


def bias_grad_ordered_rows(M):
    """rows of the partials scratch of bias_grad_ordered for M rows of dy (host-side sizing: no GPU needed)."""
    return int(_lib.lib.vacnic_bias_grad_ordered_rows(M))


def bias_grad_ordered(dy2d, dbias, M, N, partials=None):
    """dbias[n] += sum_m dy[m][n] without atomics: per-row-block column sums, then the ordered fold (vacnic_bias_grad_ordered)."""
    rows = bias_grad_ordered_rows(M)
    if partials is None:
        partials = torch.empty((rows, max(N, 1)), device=dy2d.device, dtype=torch.float32)
    call("vacnic_bias_grad_ordered", _p(dy2d), _p(dbias), M, N, dy2d.stride(0), _p(partials), partials.shape[0], _stream())


def scatter_ordered(src, ids, dembed, dpos, T, V, pos_offset=2, padding_idx=1, scale=1.0):
    """dembed[id] += scale * (sum of the rows of src with that id, ascending), dpos[t + pos_offset] += sum of rows t, t + T, ...
    (vacnic_scatter_ordered); src fp32 [R, D], ids int64 [R]; either destination may be None."""
    R, D = src.shape
    assert src.dtype == torch.float32 and src.is_contiguous() and ids.dtype == torch.int64 and ids.numel() == R
    call("vacnic_scatter_ordered", _p(src), _p(ids), _p(dembed), _p(dpos), R, T, D, V, pos_offset, padding_idx, float(scale), _stream())


def ce_bwd(logits, targets, V, row_lse, acc, dlogits, grad_out=None, grad_scale=1.0, ignore_index=1, label_smoothing=0.0):
    R, ldl = logits.shape[0], logits.stride(0)
    call_struct("vacnic_ce_bwd", stream=_stream(), logits=_p(logits), targets=_p(targets), row_lse=_p(row_lse),
                row_loss=None, loss_sum=acc.data_ptr(), count=acc.data_ptr() + 4, dlogits=_p(dlogits),
                grad_out=_p(grad_out), grad_scale=grad_scale, R=R, V=V, ldl=ldl, ldd=dlogits.stride(0),
                ignore_index=ignore_index, logits_f32=int(logits.dtype == torch.float32), label_smoothing=label_smoothing)


def zero_(t):
    """t.zero_() as a memset node on the launch stream (no fill kernel)."""
    assert t.is_contiguous()
    call("vacnic_zero_bytes", _p(t), t.numel() * t.element_size(), _stream())
    return t


def _lmhead_args(h2, emb16, targets, V, ignore_index, part=None, tl=None, row_lse=None, acc=None, bias=None, part_sum=None,
                 label_smoothing=0.0):
    R, D = h2.shape
    return _lib.LmheadCeArgs(h=_p(h2), emb=_p(emb16), bias=_p(bias), targets=_p(targets), part=_p(part), tl=_p(tl), row_lse=_p(row_lse),
                             loss_sum=acc.data_ptr() if acc is not None else None, count=acc.data_ptr() + 4 if acc is not None else None,
                             R=R, V=V, D=D, ldh=h2.stride(0), lde=emb16.stride(0), part_tiles=(V + 255) // 256, ignore_index=ignore_index,
                             part_sum=_p(part_sum), label_smoothing=label_smoothing)


def lmhead_ce_fwd(h2, emb16, targets, V, ignore_index=1, label_smoothing=0.0, bias=None, part_sum=None):
    """fused lm_head + CrossEntropyLoss forward without logits: returns (row_lse [R], acc = {loss_sum, count}).
    label_smoothing > 0: torch's CrossEntropyLoss(label_smoothing=) — the epilogue also keeps the per-tile sums of the logits in
    `part_sum` ([R, ceil(V / 256)] f32 scratch, allocated when not given); 0.0 is the plain path and never touches it.
    bias: optional f32 [V] (final_logits_bias).
    Domain: targets in [0, V) or equal to ignore_index; anything else is undefined on the fused path."""
    R = h2.shape[0]
    dev = h2.device
    tiles = (V + 255) // 256
    part = torch.empty((R, tiles, 2), device=dev, dtype=torch.float32)
    tl = torch.empty(R, device=dev, dtype=torch.float32)
    row_lse = torch.empty(R, device=dev, dtype=torch.float32)
    acc = torch.empty(2, device=dev, dtype=torch.float32)
    if label_smoothing > 0.0 and part_sum is None:
        part_sum = torch.empty((R, tiles), device=dev, dtype=torch.float32)
    if part_sum is not None and (tuple(part_sum.shape) != (R, tiles) or part_sum.dtype != torch.float32 or not part_sum.is_contiguous()
                                 or part_sum.device != dev):
        raise ValueError(f"lmhead_ce_fwd: part_sum must be a contiguous float32 [{R}, {tiles}] tensor on {dev}")
    if DETERMINISTIC:
        return lmhead_ce_fwd_ordered(h2, emb16, targets, V, part, tl, row_lse, ignore_index, label_smoothing, bias, part_sum)[:2]
    st = _lmhead_args(h2, emb16, targets, V, ignore_index, part, tl, row_lse, acc, bias=bias, part_sum=part_sum,
                      label_smoothing=label_smoothing)
    _lib.check(_lib.lib.vacnic_lmhead_ce_fwd(_lib.C.byref(st), _stream()))
    return row_lse, acc


def lmhead_ce_fwd_ordered(h2, emb16, targets, V, part, tl, row_lse, ignore_index, label_smoothing, bias, part_sum):
    """lmhead_ce_fwd in the deterministic mode -> (row_lse, acc, row_loss).  The forward entry point runs as it is (row_lse and
    `count`, a sum of 1.0s, are its own: bit-identical) with its loss atomics pointed at a word nobody reads; the per-row loss terms
    are then formed from what it left behind (vacnic_lmhead_row_loss) and summed in a fixed order into loss_sum."""
    R = h2.shape[0]
    dev = h2.device
    acc = torch.empty(4, device=dev, dtype=torch.float32)                 # {loss_sum, count, the entry point's atomic loss sum, -}
    row_loss = torch.empty(R, device=dev, dtype=torch.float32)
    st = _lmhead_args(h2, emb16, targets, V, ignore_index, part, tl, row_lse, acc, bias=bias, part_sum=part_sum,
                      label_smoothing=label_smoothing)
    st.loss_sum = acc.data_ptr() + 8
    _lib.check(_lib.lib.vacnic_lmhead_ce_fwd(_lib.C.byref(st), _stream()))
    call("vacnic_lmhead_row_loss", _p(row_lse), _p(tl), _p(targets), _p(part_sum) if label_smoothing > 0.0 else None, R, V, (V + 255) // 256,
         ignore_index, float(label_smoothing), _p(row_loss), _stream())
    sum_ordered(row_loss, acc)
    return row_lse, acc, row_loss


LOSS_NORMS = {"tokens": 0, "weights": 1}          # norm_mode of vacnic_lmhead_ce_wloss


def check_loss_weights(who, weights, R, rows_per_weight, device, norm="tokens"):
    """ValueError (naming the offending value) unless `weights` is what the weighted LM-head calls read: a contiguous float32 tensor
    of R / rows_per_weight elements on `device`, and norm one of LOSS_NORMS.  Host-side only: nothing is launched."""
    if norm not in LOSS_NORMS:
        raise ValueError(f"{who}: norm={norm!r} is not one of {sorted(LOSS_NORMS)}")
    if not isinstance(weights, torch.Tensor):
        raise ValueError(f"{who}: weights must be a float32 tensor, got {type(weights).__name__}")
    if weights.dtype != torch.float32:
        raise ValueError(f"{who}: weights must be float32, got {weights.dtype}")
    if weights.device != device:
        raise ValueError(f"{who}: weights live on {weights.device}, the hidden states on {device}")
    if not weights.is_contiguous():
        raise ValueError(f"{who}: weights must be contiguous, got strides {tuple(weights.stride())} for shape {tuple(weights.shape)}")
    if not isinstance(rows_per_weight, int) or rows_per_weight < 1 or R % rows_per_weight != 0:
        raise ValueError(f"{who}: rows_per_weight={rows_per_weight!r} does not divide the {R} rows")
    if weights.numel() != R // rows_per_weight:
        raise ValueError(f"{who}: weights hold {weights.numel()} elements, {R} rows / rows_per_weight {rows_per_weight} need "
                         f"{R // rows_per_weight}")


def lmhead_ce_fwd_weighted(h2, emb16, targets, V, weights, rows_per_weight=1, norm="tokens", ignore_index=1, label_smoothing=0.0,
                           bias=None):
    """fused lm_head + weighted cross entropy forward without logits -> (row_lse [R], acc = {sum_r w_r l_r, N}, row_nll [R]) with
    w_r = weights[r // rows_per_weight] (fp32, any sign), l_r the row's unweighted loss term (row_nll, an exact 0 on ignored rows)
    and N the number of non-ignored rows (norm "tokens") or the sum of their weights (norm "weights").  loss = acc[0] / acc[1].
    The forward entry point runs as it is, its atomics pointed at words nobody reads (as in lmhead_ce_fwd_ordered); the weighted
    sums are formed from what it left behind in a fixed order (vacnic_lmhead_ce_wloss): the same bits in every run and mode.
    Domain: targets in [0, V) or equal to ignore_index; anything else is undefined on the fused path."""
    R = h2.shape[0]
    dev = h2.device
    check_loss_weights("lmhead_ce_fwd_weighted", weights, R, rows_per_weight, dev, norm)
    tiles = (V + 255) // 256
    part = torch.empty((R, tiles, 2), device=dev, dtype=torch.float32)
    tl = torch.empty(R, device=dev, dtype=torch.float32)
    row_lse = torch.empty(R, device=dev, dtype=torch.float32)
    part_sum = torch.empty((R, tiles), device=dev, dtype=torch.float32) if label_smoothing > 0.0 else None
    acc = torch.empty(4, device=dev, dtype=torch.float32)                 # {sum w l, N, the entry point's atomic loss sum, its count}
    rows = torch.empty((3, R), device=dev, dtype=torch.float32)           # row_nll, row_wloss, row_wnorm
    st = _lmhead_args(h2, emb16, targets, V, ignore_index, part, tl, row_lse, acc, bias=bias, part_sum=part_sum,
                      label_smoothing=label_smoothing)
    st.loss_sum, st.count = acc.data_ptr() + 8, acc.data_ptr() + 12
    _lib.check(_lib.lib.vacnic_lmhead_ce_fwd(_lib.C.byref(st), _stream()))
    call("vacnic_lmhead_ce_wloss", _p(row_lse), _p(tl), _p(targets), _p(part_sum), _p(weights), rows_per_weight, R, V, tiles, ignore_index,
         float(label_smoothing), LOSS_NORMS[norm], _p(rows[0]), _p(rows[1]), _p(rows[2]), _p(acc), _stream())
    return row_lse, acc, rows[0]


LmheadEval = collections.namedtuple("LmheadEval", "row_lse row_nll pred seq_nll seq_tokens seq_correct")


def lmhead_eval(h2, emb16, targets, V, rows_per_seq, ignore_index=1, bias=None, totals=None):
    """fused validation head: ONE lm_head pass without logits -> LmheadEval(row_lse [R] f32 (bit-identical to lmhead_ce_fwd's),
    row_nll [R] f32 (lse - target logit; exact 0 where target == ignore_index), pred [R] int64 (argmax over the V real columns, ties
    to the lowest index), seq_nll [S] f32, seq_tokens [S] int32, seq_correct [S] int32) with S = R / rows_per_seq captions of
    rows_per_seq consecutive rows each.  totals: optional float64 [4] running record {nll, tokens, correct, sequences} the call
    ADDS its sums to (zero it once per validation pass with zero_()).  No fp32 atomics: every output is bit-reproducible.
    Domain: targets in [0, V) or equal to ignore_index; anything else is undefined on the fused path."""
    R = h2.shape[0]
    dev = h2.device
    tiles = (V + 255) // 256
    if totals is not None and (tuple(totals.shape) != (4,) or totals.dtype != torch.float64 or not totals.is_contiguous() or totals.device != dev):
        raise ValueError(f"lmhead_eval: totals must be a contiguous float64 [4] tensor on {dev}")
    S = R // rows_per_seq if rows_per_seq > 0 else 0                  # (a bad rows_per_seq is the library's to reject)
    part = torch.empty((R, tiles, 2), device=dev, dtype=torch.float32)
    part_arg = torch.empty((R, tiles), device=dev, dtype=torch.int32)
    tl = torch.empty(R, device=dev, dtype=torch.float32)
    out = LmheadEval(row_lse=torch.empty(R, device=dev, dtype=torch.float32), row_nll=torch.empty(R, device=dev, dtype=torch.float32),
                     pred=torch.empty(R, device=dev, dtype=torch.int64), seq_nll=torch.empty(max(S, 1), device=dev, dtype=torch.float32)[:S],
                     seq_tokens=torch.empty(max(S, 1), device=dev, dtype=torch.int32)[:S],
                     seq_correct=torch.empty(max(S, 1), device=dev, dtype=torch.int32)[:S])
    lmhead_eval_into(h2, emb16, targets, V, rows_per_seq, part, part_arg, tl, out, ignore_index=ignore_index, bias=bias, totals=totals)
    return out


def lmhead_eval_into(h2, emb16, targets, V, rows_per_seq, part, part_arg, tl, out, ignore_index=1, bias=None, totals=None, part_tiles=None):
    """vacnic_lmhead_eval on caller-owned scratch (part, part_arg, tl) and outputs (an LmheadEval record): what a launch plan
    records.  part_tiles: the tile count to declare (default ceil(V / 256), the only value the library accepts)."""
    R, D = h2.shape
    st = _lib.LmheadEvalArgs(h=_p(h2), emb=_p(emb16), bias=_p(bias), targets=_p(targets), part=_p(part), part_arg=_p(part_arg), tl=_p(tl),
                             row_lse=_p(out.row_lse), row_nll=_p(out.row_nll), pred=_p(out.pred), seq_nll=_p(out.seq_nll),
                             seq_tokens=_p(out.seq_tokens), seq_correct=_p(out.seq_correct), totals=_p(totals),
                             R=R, V=V, D=D, ldh=h2.stride(0), lde=emb16.stride(0),
                             part_tiles=(V + 255) // 256 if part_tiles is None else part_tiles, ignore_index=ignore_index,
                             rows_per_seq=rows_per_seq)
    _lib.check(_lib.lib.vacnic_lmhead_eval(_lib.C.byref(st), _stream()))


def lmhead_ce_rowp(row_lse, targets, acc, grad_out=None, grad_scale=1.0, ignore_index=1, label_smoothing=0.0, V=None, weights=None,
                   rows_per_weight=1):
    """per-row operands of lmhead_ce_dlogits: [R, 2] = {lse, coef}; with label_smoothing > 0 (which needs V) [R, 4] =
    {lse, coef, coef (1 - eps), coef eps / V}.  Pass the same label_smoothing to lmhead_ce_dlogits.
    weights (fp32 [R / rows_per_weight], with the acc of lmhead_ce_fwd_weighted): coef = (grad_out grad_scale / acc[1]) * w_r, acc[1]
    used as it is; acc[1] <= 0 or non-finite gives all-zero coefficients (vacnic_lmhead_ce_rowp_w).
    Domain: targets in [0, V) or equal to ignore_index; anything else is undefined on the fused path."""
    R = row_lse.shape[0]
    if weights is not None:
        check_loss_weights("lmhead_ce_rowp", weights, R, rows_per_weight, row_lse.device)
        if label_smoothing != 0.0 and V is None:
            raise TypeError("lmhead_ce_rowp: label_smoothing needs V (the uniform term is eps / V)")
        rowp = torch.empty((R, 4 if label_smoothing > 0.0 else 2), device=row_lse.device, dtype=torch.float32)
        call("vacnic_lmhead_ce_rowp_w", _p(row_lse), _p(targets), _p(weights), rows_per_weight, acc.data_ptr() + 4, _p(grad_out), grad_scale,
             float(label_smoothing), 1 if V is None else V, _p(rowp), R, ignore_index, _stream())
        return rowp
    if label_smoothing != 0.0:
        if V is None:
            raise TypeError("lmhead_ce_rowp: label_smoothing needs V (the uniform term is eps / V)")
        rowp = torch.empty((R, 4), device=row_lse.device, dtype=torch.float32)
        call("vacnic_lmhead_ce_rowp_smooth", _p(row_lse), _p(targets), acc.data_ptr() + 4, _p(grad_out), grad_scale, label_smoothing, V,
             _p(rowp), R, ignore_index, _stream())
        return rowp
    rowp = torch.empty((R, 2), device=row_lse.device, dtype=torch.float32)
    call("vacnic_lmhead_ce_rowp", _p(row_lse), _p(targets), acc.data_ptr() + 4, _p(grad_out), grad_scale, _p(rowp), R, ignore_index, _stream())
    return rowp


def lmhead_ce_dlogits(h2, emb16, targets, V, rowp, dl, col0, ncols, ignore_index=1, label_smoothing=0.0, bias=None):
    """dl[:, :round_up(ncols, 8)] = bf16 dlogits of vocabulary columns [col0, col0 + ncols) (logits recomputed on chip).
    Domain: targets in [0, V) or equal to ignore_index; anything else is undefined on the fused path."""
    if 0.0 <= label_smoothing < 1.0 and rowp.shape[-1] != (4 if label_smoothing > 0.0 else 2):   # (a bad eps is the library's to reject)
        raise ValueError(f"lmhead_ce_dlogits: rowp has {rowp.shape[-1]} floats per row; label_smoothing={label_smoothing} reads "
                         f"{4 if label_smoothing > 0.0 else 2} (build it with lmhead_ce_rowp(label_smoothing=...))")
    st = _lmhead_args(h2, emb16, targets, V, ignore_index, bias=bias, label_smoothing=label_smoothing)
    _lib.check(_lib.lib.vacnic_lmhead_ce_dlogits(_lib.C.byref(st), col0, ncols, _p(dl), dl.stride(0), _p(rowp), _stream()))


def combine_losses(ce_sum_ptr, count_ptr, secla, colam, w_secla, w_colam, device):
    out4 = torch.empty(4, device=device, dtype=torch.float32)
    call("vacnic_combine_losses", ce_sum_ptr, count_ptr, _p(secla), _p(colam), w_secla, w_colam, out4.data_ptr(), _stream())
    return out4


def colam_fwd(hs, hg, mask_u8, margin):
    B, T, D = hs.shape
    dev = hs.device
    loss = torch.empty((), device=dev, dtype=torch.float32)
    cos = torch.empty(B, device=dev, dtype=torch.float32)
    ps = torch.empty((B, D), device=dev, dtype=torch.float32)
    pg = torch.empty((B, D), device=dev, dtype=torch.float32)
    call_struct("vacnic_colam_fwd", stream=_stream(), hs=_p(hs), hg=_p(hg), mask=_p(mask_u8), loss=_p(loss), cos=_p(cos),
                pooled_s=_p(ps), pooled_g=_p(pg), B=B, T=T, D=D, margin=margin)
    return loss, cos, ps, pg


def colam_bwd(cos, ps, pg, mask_u8, shape, margin, grad_out, grad_scale):
    B, T, D = shape
    dhs = torch.empty(shape, device=cos.device, dtype=BF16)
    call_struct("vacnic_colam_bwd", stream=_stream(), cos=_p(cos), pooled_s=_p(ps), pooled_g=_p(pg), mask=_p(mask_u8),
                dhs=_p(dhs), B=B, T=T, D=D, margin=margin, grad_out=_p(grad_out), grad_scale=grad_scale)
    return dhs


def secla_fwd(faces, names):
    B, F, D = faces.shape
    N = names.shape[1]
    dev = faces.device
    sim = torch.empty((B, N, B, F), device=dev, dtype=torch.float32)
    l1 = torch.empty((B, B), device=dev, dtype=torch.float32)
    l2 = torch.empty((B, B), device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    call_struct("vacnic_secla_fwd", stream=_stream(), faces=_p(faces), names=_p(names), sim=_p(sim), logits1=_p(l1),
                logits2=_p(l2), loss=_p(loss), B=B, F=F, N=N, D=D)
    return loss, sim, l1, l2


def secla_bwd(faces, names, sim, l1, l2, grad_out, grad_scale):
    B, F, D = faces.shape
    N = names.shape[1]
    dfaces = torch.empty((B, F, D), device=faces.device, dtype=BF16)
    wsim = torch.empty_like(sim)
    call_struct("vacnic_secla_bwd", stream=_stream(), faces=_p(faces), names=_p(names), sim=_p(sim), logits1=_p(l1),
                logits2=_p(l2), dfaces=_p(dfaces), wsim=_p(wsim), B=B, F=F, N=N, D=D, grad_out=_p(grad_out),
                grad_scale=grad_scale)
    return dfaces


# ---------------------------------------------------------------------------------------------- optimizer
def lr_step(hyper, base_lr, warmup, total, rng_counter=None):
    call("vacnic_lr_step", hyper.data_ptr(), base_lr, float(warmup), float(total), _p(rng_counter), _stream())


def accum_state(device):
    """the int64[4] state of lr_step_accum(): {step word, micro-batches pending, groups completed, 0}."""
    return torch.zeros(4, device=device, dtype=torch.int64)


def lr_step_accum(hyper, base_lr, warmup, total, accum, k, rng_counter=None):
    """lr_step() for k micro-batches per optimizer step, counted on the device: every call advances the dropout counter; the first
    k - 1 calls of a group set accum[0] = 2 (hold) and leave hyper alone, the k-th sets it to 0 and advances hyper as lr_step does.
    Pass accum as `hold` to grad_guard / grad_clip_coef_groups and as `skip` to param_stats / adamw* (with a guard: its state)."""
    assert accum.dtype == torch.int64 and accum.numel() >= 4
    call("vacnic_lr_step_accum", hyper.data_ptr(), base_lr, float(warmup), float(total), _p(rng_counter), _p(accum), int(k), _stream())


def _adamw_fields(p, g, m, v, p16, hyper, n, beta1, beta2, eps, grad_scale, zero_grad, clip_coef, skip):
    """the struct fields that vacnic_adamw, vacnic_adamw_groups and vacnic_adamw_ema have in common."""
    return dict(p=_p(p), g=_p(g), m=_p(m), v=_p(v), p_bf16=_p(p16), hyper=_p(hyper), n=n, beta1=beta1, beta2=beta2, eps=eps,
                grad_scale=grad_scale, zero_grad=int(zero_grad), clip_coef=_p(clip_coef), skip=_p(skip))


def _group_table(table, elem_base):
    """struct fields of a device-resident parameter-group table (arena.group_table(...).to(device)); None: the null table, which
    the entry points that take it as an option read as "ungrouped"."""
    if table is None:
        return dict(seg_start=None, seg=None, first_seg=None, nseg=0, nblocks=0, elem_base=elem_base)
    return dict(seg_start=_p(table.seg_start), seg=_p(table.seg), first_seg=_p(table.first_seg), nseg=table.nseg,
                nblocks=table.first_seg.numel(), elem_base=elem_base)


def _norm_scratch(g, partials, out):
    """the norm passes' scratch (1024 partial sums) and result {clip coefficient, total norm}, allocated where not given."""
    if partials is None:
        partials = torch.empty(1024, device=g.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(2, device=g.device, dtype=torch.float32)
    assert g.dtype == torch.float32 and partials.numel() >= 1024 and out.numel() >= 2
    return partials, out


def adamw(p, g, m, v, p16, hyper, n, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, zero_grad=True,
          clip_coef=None, skip=None):
    """skip: the int64 state of grad_guard() or of lr_step_accum() (or None): when its word is 1 the step only zeroes g, when it is 2
    (a held micro-batch) the step does nothing at all."""
    call_struct("vacnic_adamw", stream=_stream(), weight_decay=weight_decay,
                **_adamw_fields(p, g, m, v, p16, hyper, n, beta1, beta2, eps, grad_scale, zero_grad, clip_coef, skip))


def grad_clip_coef(g, n, max_norm, grad_scale=1.0, partials=None, out=None):
    """clip_grad_norm_ (TRAIN:365-366) on device: returns the fp32 pair {clip coefficient, total norm}."""
    partials, out = _norm_scratch(g, partials, out)
    call("vacnic_grad_clip_coef", _p(g), n, grad_scale, max_norm, _p(partials), _p(out), _stream())
    return out


def adamw_groups(p, g, m, v, p16, hyper, n, table, elem_base=0, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, zero_grad=True,
                 clip_coef=None, skip=None):
    """adamw() with per-segment lr multiple / weight decay / frozen flag; p, g, m, v, p16 start at arena element elem_base."""
    call_struct("vacnic_adamw_groups", stream=_stream(), **_group_table(table, elem_base),
                **_adamw_fields(p, g, m, v, p16, hyper, n, beta1, beta2, eps, grad_scale, zero_grad, clip_coef, skip))


def adamw_ema(p, g, m, v, p16, hyper, n, ema, ema_decay, ema_warmup=True, table=None, elem_base=0, beta1=0.9, beta2=0.999, eps=1e-8,
              weight_decay=0.01, grad_scale=1.0, zero_grad=True, clip_coef=None, skip=None):
    """adamw() (table=None: `weight_decay`) or adamw_groups() (a table) that also keeps `ema`, laid out like p, in the same pass:
    ema = d * ema + (1 - d) * p_new with d = ema_decay, under ema_warmup min(ema_decay, (1 + t) / (10 + t)) for Adam's step t.
    Frozen segments and a skipped step leave ema as it is."""
    assert ema.dtype == torch.float32
    call_struct("vacnic_adamw_ema", stream=_stream(), weight_decay=weight_decay, ema=_p(ema), ema_decay=float(ema_decay),
                ema_warmup=int(bool(ema_warmup)), **_group_table(table, elem_base),
                **_adamw_fields(p, g, m, v, p16, hyper, n, beta1, beta2, eps, grad_scale, zero_grad, clip_coef, skip))


def ema_swap(p, ema, p16=None):
    """exchange the contents of p and ema (fp32, same size, a multiple of 4) and refresh the bf16 shadow p16 from the new p."""
    assert p.dtype == torch.float32 and ema.dtype == torch.float32 and p.numel() == ema.numel()
    assert p.is_contiguous() and ema.is_contiguous() and (p16 is None or (p16.is_contiguous() and p16.numel() == p.numel()))
    call("vacnic_ema_swap", _p(p), _p(ema), _p(p16), p.numel(), _stream())


def grad_clip_coef_groups(g, n, max_norm, table, grad_scale=1.0, partials=None, out=None, elem_base=0, hold=None):
    """grad_clip_coef() over the non-frozen segments of the table (None: ungrouped).  hold: the state of lr_step_accum() or None;
    on a held micro-batch the arena is not read and `out` stays."""
    partials, out = _norm_scratch(g, partials, out)
    call_struct("vacnic_grad_clip_coef_groups", stream=_stream(), g=_p(g), n=n, grad_scale=grad_scale, max_norm=max_norm,
                partials=_p(partials), out=_p(out), hold=_p(hold), **_group_table(table, elem_base))
    return out


def guard_state(device):
    """the int64[4] state of grad_guard(): {skip flag, skipped total, consecutive skips, first non-finite index (-1: none)}."""
    return torch.tensor([0, 0, 0, -1], device=device, dtype=torch.int64)


def grad_guard(g, n, hyper, state=None, max_norm=0.0, table=None, grad_scale=1.0, partials=None, first_idx=None, out=None,
               elem_base=0, hold=None):
    """Non-finite gradient guard on device (no sync): call between lr_step() and adamw(skip=state).  Writes out = {clip coefficient,
    norm} as grad_clip_coef[_groups] does (max_norm <= 0: coefficient 1), the verdict and counters into `state`, and on a skip takes
    lr_step's increment of hyper[1] back.  table: a parameter-group table (frozen segments are left out) or None.
    hold: the state of lr_step_accum() or None; on a held micro-batch the guard only writes state[0] = 2.
    Returns (out, state)."""
    if state is None:
        state = guard_state(g.device)
    if first_idx is None:
        first_idx = torch.empty(1024, device=g.device, dtype=torch.int64)
    partials, out = _norm_scratch(g, partials, out)
    assert first_idx.dtype == torch.int64 and first_idx.numel() >= 1024 and state.dtype == torch.int64 and state.numel() >= 4
    call_struct("vacnic_grad_guard", stream=_stream(), g=_p(g), n=n, grad_scale=grad_scale, max_norm=float(max_norm),
                partials=_p(partials), first_idx=_p(first_idx), out=_p(out), state=_p(state), hyper=_p(hyper),
                hold=_p(hold), **_group_table(table, elem_base))
    return out, state


def param_stats_workspace(table, device):
    """the caller-owned scratch of param_stats() for this table (the unit partials of pass 1)."""
    nbytes = int(_lib.lib.vacnic_param_stats_workspace_bytes(table.nunit, table.nslot))
    return torch.empty(nbytes, device=device, dtype=torch.uint8)


def param_stats(g, p, n, table, hyper=None, every=1, skip=None, grad_scale=1.0, workspace=None, out_f=None, out_i=None, stamp=None):
    """Per-slot statistics of the gradient arena g (and the weights p, or None) on device, gated on device (no sync): fires when
    hyper is None, when int(hyper[1]) % every == 0, or when skip (grad_guard's state) is 1; otherwise, and always on a held
    micro-batch (skip's word is 2: grad_guard's or lr_step_accum's state), nothing is written.
    table: arena.stats_table(...).to(device).  out_f float[nslot][4] = {sum x^2, max |x| over finite x = g * grad_scale, sum p^2,
    max |p|}, out_i int64[nslot][2] = {non-finite elements, elements with g == 0}, stamp int64[4] = {fires so far, hyper[1] as
    read, fired on a skip, 0}; allocated (zeroed) where not given.  Returns (out_f, out_i, stamp)."""
    if workspace is None:
        workspace = param_stats_workspace(table, g.device)
    if out_f is None:
        out_f = torch.zeros(table.nslot, 4, device=g.device, dtype=torch.float32)
    if out_i is None:
        out_i = torch.zeros(table.nslot, 2, device=g.device, dtype=torch.int64)
    if stamp is None:
        stamp = torch.zeros(4, device=g.device, dtype=torch.int64)
    assert g.dtype == torch.float32 and (p is None or p.dtype == torch.float32)
    assert out_f.dtype == torch.float32 and out_f.numel() >= 4 * table.nslot and out_f.is_contiguous()
    assert out_i.dtype == torch.int64 and out_i.numel() >= 2 * table.nslot and out_i.is_contiguous()
    assert stamp.dtype == torch.int64 and stamp.numel() >= 4
    call_struct("vacnic_param_stats", stream=_stream(), g=_p(g), p=_p(p), n=n, grad_scale=grad_scale, unit_off=_p(table.unit_off),
                unit_len=_p(table.unit_len), nunit=table.nunit, slot_unit=_p(table.slot_unit), nslot=table.nslot, hyper=_p(hyper),
                every=int(every), skip=_p(skip), workspace=_p(workspace), workspace_bytes=workspace.numel() * workspace.element_size(),
                out_f=_p(out_f), out_i=_p(out_i), stamp=_p(stamp))
    return out_f, out_i, stamp


# ------------------------------------------------------------------------------------------------- misc
def cast_f32_bf16(src, dst=None):
    if dst is None:
        dst = torch.empty(src.shape, device=src.device, dtype=BF16)
    assert src.is_contiguous() and dst.is_contiguous()
    call("vacnic_cast_f32_bf16", _p(src), _p(dst), src.numel(), _stream())
    return dst


def cast_bf16_f32(src, dst=None):
    if dst is None:
        dst = torch.empty(src.shape, device=src.device, dtype=torch.float32)
    assert src.is_contiguous() and dst.is_contiguous()
    call("vacnic_cast_bf16_f32", _p(src), _p(dst), src.numel(), _stream())
    return dst


def copy3d(src, dst, B, rows, cols, accumulate=False):
    """src/dst: [B, rows, cols] views with unit inner stride."""
    call("vacnic_copy3d_bf16", _p(src), _p(dst), B, rows, cols, src.stride(1), dst.stride(1), src.stride(0), dst.stride(0),
         int(accumulate), _stream())


def zero_strided(t):
    """zero a [B, rows, cols] bf16 view with unit inner stride (rare fallback: an unused slot of a batched gradient buffer)."""
    z = torch.empty((t.shape[0], t.shape[1], t.shape[2]), device=t.device, dtype=t.dtype)
    zero_(z)
    copy3d(z, t, t.shape[0], t.shape[1], t.shape[2])


def cat_tokens(parts):
    """torch.cat(parts, dim=1) for [B, T_i, D] bf16 tensors (MFULL:666,691)."""
    B, _, D = parts[0].shape
    T = sum(p.shape[1] for p in parts)
    out = torch.empty((B, T, D), device=parts[0].device, dtype=BF16)
    o = 0
    for p in parts:
        copy3d(p, out[:, o:o + p.shape[1]], B, p.shape[1], D)
        o += p.shape[1]
    return out


def pad_cols(x2d, Cp):
    """[R, C] -> [R, Cp] zero padded (C not a multiple of 8)."""
    R, C = x2d.shape
    out = torch.empty((R, Cp), device=x2d.device, dtype=BF16)
    call("vacnic_pad_cols_bf16", _p(x2d), _p(out), R, C, Cp, x2d.stride(0), _stream())
    return out


def add(a, b):
    out = torch.empty_like(a)
    assert a.is_contiguous() and b.is_contiguous()
    call("vacnic_add_bf16", _p(a), _p(b), _p(out), a.numel(), _stream())
    return out


def im2col_patches(img, patch, Kp):
    B, _, HW, _ = img.shape
    g = HW // patch
    out = torch.empty((B * g * g, Kp), device=img.device, dtype=BF16)
    call("vacnic_im2col_patches", _p(img), _p(out), B, HW, patch, Kp, _stream())
    return out


def vit_assemble(patch_emb, cls16, pos16, B, G2, W):
    out = torch.empty((B, G2 + 1, W), device=patch_emb.device, dtype=BF16)
    call("vacnic_vit_assemble", _p(patch_emb), _p(cls16), _p(pos16), _p(out), B, G2, W, _stream())
    return out


def prep_ids(ids, pad_id=1, start_id=None, want_mask=True):
    B, T = ids.shape
    mask = torch.empty((B, T), device=ids.device, dtype=torch.uint8) if want_mask else None
    shifted = torch.empty_like(ids) if start_id is not None else None
    call("vacnic_prep_ids", _p(ids), _p(mask), _p(shifted), B, T, pad_id, start_id if start_id is not None else 0, _stream())
    return mask, shifted


def prep_ids_into(ids, mask, shifted, pad_id=1, start_id=None):
    """prep_ids writing into caller-owned buffers (either may be None)."""
    B, T = ids.shape
    call("vacnic_prep_ids", _p(ids), _p(mask), _p(shifted), B, T, pad_id, start_id if start_id is not None else 0, _stream())


def face_mask(face_emb):
    B, F, D = face_emb.shape
    mask = torch.empty((B, F), device=face_emb.device, dtype=torch.uint8)
    call("vacnic_face_mask", _p(face_emb), _p(mask), B * F, D, _stream())
    return mask


def cat_masks(a, b):
    """torch.cat((a, b), dim=1) for two uint8 [B, n] masks (MFULL:1262)."""
    assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.is_contiguous() and b.is_contiguous() and a.shape[0] == b.shape[0]
    out = torch.empty((a.shape[0], a.shape[1] + b.shape[1]), device=a.device, dtype=torch.uint8)
    call("vacnic_cat2_u8", _p(a), _p(b), _p(out), a.shape[0], a.shape[1], b.shape[1], _stream())
    return out


def argmax_rows(logits, V):
    R = logits.shape[0]
    out = torch.empty(R, device=logits.device, dtype=torch.int64)
    call("vacnic_argmax_rows", _p(logits), _p(out), R, V, logits.stride(0), int(logits.dtype == torch.float32), _stream())
    return out


def bias_grad(dy2d, dbias, M, N):
    if DETERMINISTIC:
        return bias_grad_ordered(dy2d, dbias, M, N)
    call("vacnic_bias_grad", _p(dy2d), _p(dbias), M, N, dy2d.stride(0), _stream())


def probe_layouts():
    out = torch.zeros(2624, device="cuda", dtype=torch.float32)
    src = torch.arange(128, device="cuda", dtype=torch.float32) + 1.0
    call("vacnic_probe_layouts", _p(out), _p(src), out.numel(), _stream())
    return out


# ------------------------------------------------------------------------------------------------ decode
PENALTY_RULES = {None: 0, "logits": 1, "scores": 2}      # penalty_rule of vacnic_beam_topk_ex / vacnic_lmhead_topk


def beam_topk(logits, V, K_, beam_scores=None, bans=None, eos=2, suppress_eos=False, forced_token=-1, history=None, cur_len=0,
              repetition_penalty=1.0, penalty_rule=None):
    """history int32 [R, >= cur_len] + repetition_penalty + penalty_rule "logits" | "scores": vacnic_beam_topk_ex (include/vacnic_hip.h)"""
    R = logits.shape[0]
    tv = torch.empty((R, K_), device=logits.device, dtype=torch.float32)
    ti = torch.empty((R, K_), device=logits.device, dtype=torch.int32)
    if penalty_rule is not None:
        call_struct("vacnic_beam_topk_ex", stream=_stream(), logits=_p(logits), beam_scores=_p(beam_scores), bans=_p(bans), top_val=_p(tv),
                    top_idx=_p(ti), history=_p(history), R=R, V=V, ldl=logits.stride(0), hist_stride=history.stride(0) if history is not None else 0,
                    n_ban=bans.shape[1] if bans is not None else 0, eos=eos, suppress_eos=int(suppress_eos), forced_token=forced_token, K=K_,
                    logits_f32=int(logits.dtype == torch.float32), cur_len=int(cur_len), penalty_rule=PENALTY_RULES[penalty_rule],
                    penalty=float(repetition_penalty))
        return tv, ti
    call("vacnic_beam_topk", _p(logits), _p(beam_scores), _p(bans), bans.shape[1] if bans is not None else 0, eos, int(suppress_eos),
         forced_token, _p(tv), _p(ti), R, V, logits.stride(0), K_, int(logits.dtype == torch.float32), _stream())
    return tv, ti


def lmhead_topk(h, emb, V, K_, *, bias=None, beam_scores=None, bans=None, eos=2, suppress_eos=False, forced_token=-1, logits=None,
                history=None, cur_len=0, repetition_penalty=1.0, penalty_rule=None):
    """(top values, top ids) [R, K_] of log_softmax(h . emb[:V]^T + bias) after the logits processors, + beam_scores — the LM head
    and vacnic_beam_topk of one decode position without the [R, V] logits (R <= 8, d_model <= 1024).  A forced position
    (forced_token >= 0) computes no logits at all.  logits: optional fp32 [R, >= V] buffer that receives them (diagnostics)."""
    R, d = h.shape
    tv = torch.empty((R, K_), device=h.device, dtype=torch.float32)
    ti = torch.empty((R, K_), device=h.device, dtype=torch.int32)
    nws = int(_lib.lib.vacnic_lmhead_topk_workspace(R, V, K_)) if forced_token < 0 else 0
    pen = {}
    if penalty_rule is not None:                     # (the scores rule parks the history tokens' logits behind the partial results)
        pen = dict(history=_p(history), hist_stride=history.stride(0) if history is not None else 0, cur_len=int(cur_len),
                   penalty_rule=PENALTY_RULES[penalty_rule], penalty=float(repetition_penalty))
        if penalty_rule == "scores" and forced_token < 0 and history is not None:
            nws += R * history.stride(0)
    ws = torch.empty(nws, device=h.device, dtype=torch.float32) if nws else None
    call_struct("vacnic_lmhead_topk", stream=_stream(), h=_p(h), emb=_p(emb), bias=_p(bias), logits=_p(logits) if forced_token < 0 else None,
                workspace=_p(ws), beam_scores=_p(beam_scores), bans=_p(bans), top_val=_p(tv), top_idx=_p(ti), R=R, V=V, d=d, ldw=emb.stride(0),
                ldl=logits.stride(0) if logits is not None else 0, workspace_floats=nws, n_ban=bans.shape[1] if bans is not None else 0, eos=eos,
                suppress_eos=int(suppress_eos), forced_token=forced_token, K2=K_, **pen)
    return tv, ti


BAD_WORDS_MAX, BAD_WORD_LEN = 1024, 16          # VACNIC_BAD_WORDS_MAX / VACNIC_BAD_WORD_LEN of include/vacnic_hip.h


def bad_words_table(words, device="cuda"):
    """the device bad-word table of include/vacnic_hip.h from a list of token-id lists: (int32 [n, BAD_WORD_LEN] padded with -1,
    int32 [n] lengths).  The capacity is checked here as the C entry points check it."""
    n = len(words)
    if n < 1 or n > BAD_WORDS_MAX or any(not 1 <= len(w) <= BAD_WORD_LEN for w in words):
        raise ValueError(f"bad_words_table: 1 .. {BAD_WORDS_MAX} words of 1 .. {BAD_WORD_LEN} tokens each")
    tab = torch.full((n, BAD_WORD_LEN), -1, dtype=torch.int32)
    for i, w in enumerate(words):
        tab[i, :len(w)] = torch.tensor([int(t) for t in w], dtype=torch.int32)
    lens = torch.tensor([len(w) for w in words], dtype=torch.int32)
    return tab.to(device), lens.to(device)


def sample_params(temperature=1.0, top_k=0, top_p=1.0, seed=0, call=0, out=None, repetition_penalty=1.0):
    """the 8-word runtime parameter block of vacnic_sample_step (include/vacnic_hip.h) as a CPU int32 tensor: [T f32, top_k i32,
    top_p f32, repetition penalty f32 (the word stays 0 without one: the kernel reads that as off), seed low, seed high, call low,
    call high].  `out`: a (pinned) int32 [8] tensor to fill instead."""
    import struct
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    pen = 0.0 if float(repetition_penalty) == 1.0 else float(repetition_penalty)
    words = struct.unpack("<8i", struct.pack("<fiffIIII", float(temperature), int(top_k), float(top_p), pen, seed & 0xFFFFFFFF, seed >> 32,
                                             call & 0xFFFFFFFF, call >> 32))
    out = torch.empty(8, dtype=torch.int32) if out is None else out
    out.copy_(torch.tensor(words, dtype=torch.int32))
    return out


def sample_step(logits, V, params, seq, done, next_ids, cur_len, *, logp=None, eos=2, pad=1, no_repeat_ngram_size=0, suppress_eos=False,
                forced_token=-1, kept=None, thr=None, mass=None, u=None, bad_words=None):
    """one position of sampling decode for every row: processors -> temperature -> top-k -> top-p -> one Philox draw, and the
    bookkeeping (next_ids int64 [R], seq int32 [R, Lmax] at column cur_len, done int32 [R], logp fp32 [R, Lmax]) in one launch.
    logits fp32 [R, >= V]; params: int32 [8] on the device (sample_params).  kept / thr / mass / u: optional per-row diagnostics.
    bad_words: (table, lengths) from bad_words_table."""
    R = logits.shape[0]
    bw = {} if bad_words is None else dict(bad_words=_p(bad_words[0]), bad_len=_p(bad_words[1]), n_bad=bad_words[1].shape[0])
    call_struct("vacnic_sample_step", stream=_stream(), logits=_p(logits), params=_p(params), seq=_p(seq), done=_p(done), next_ids=_p(next_ids),
                logp=_p(logp), kept=_p(kept), thr=_p(thr), mass=_p(mass), u=_p(u), R=R, V=V, ldl=logits.stride(0), Lmax=seq.shape[1],
                cur_len=int(cur_len), eos=eos, pad=pad, no_repeat_ngram_size=no_repeat_ngram_size, suppress_eos=int(bool(suppress_eos)),
                forced_token=forced_token, **bw)


def image_u8_normalize(img_u8, flip=None, mean=(0.48145466, 0.4578275, 0.40821073), std=(0.26862954, 0.26130258, 0.27577711)):
    """uint8 [B,3,H,W] (+ optional uint8 flip flags [B]) -> fp32 ToTensor + Normalize (TRAIN:741-764), bit-identical to torch."""
    B, C, H, W = img_u8.shape
    assert C == 3 and img_u8.dtype == torch.uint8 and img_u8.is_contiguous()
    out = torch.empty((B, 3, H, W), device=img_u8.device, dtype=torch.float32)
    call("vacnic_image_u8_normalize", _p(img_u8), _p(flip), _p(out), B, H, W, *[float(v) for v in mean], *[float(v) for v in std], _stream())
    return out


def gather_rows(src, dst, idx, rows, row_bytes, row_stride_bytes=0, period=0):
    call("vacnic_gather_rows", _p(src), _p(dst), _p(idx), rows, row_bytes, row_stride_bytes, period, _stream())


def group_beam_args(groups, forced_token=-1, repetition_penalty=1.0, penalty_rule=None):
    """vacnic_group_beam_args from groups = (num_beam_groups, diversity_penalty) and the processors of the position's top-k call"""
    if penalty_rule == "logits":
        raise ValueError("group beam search: the repetition penalty is on the scores (more than one beam), never on the logits")
    return _lib.GroupBeamArgs(num_beam_groups=int(groups[0]), diversity_penalty=float(groups[1]), repetition_penalty=float(repetition_penalty),
                              penalty_rule=PENALTY_RULES[penalty_rule], forced_token=int(forced_token))


def beam_alloc(B, nb, Lmax, V, eos, pad, no_repeat_ngram_size=0, early_stopping=False, length_penalty=1.0, device="cuda", bad_words=None,
               groups=None):
    """the device state of vacnic_beam_init / vacnic_beam_step (include/vacnic_hip.h) as a namespace of tensors + the C struct `st`.
    bad_words: (table, lengths) from bad_words_table; the ban lists are then Lmax + n_bad wide.
    groups = (num_beam_groups, diversity_penalty): the same state serves vacnic_group_beam_init / vacnic_group_beam_step (group_beam_init /
    group_beam_step below read it from `s.groups`); None = ordinary beams."""
    import types
    if groups is not None and (int(groups[0]) < 1 or nb % int(groups[0]) != 0):
        raise ValueError(f"beam_alloc: num_beam_groups {groups[0]} must be >= 1 and divide nb = {nb}")
    R = B * nb
    n_bad = 0 if bad_words is None else int(bad_words[1].shape[0])
    bw = {} if bad_words is None else dict(bad_words=_p(bad_words[0]), bad_len=_p(bad_words[1]), n_bad=n_bad)
    i32 = dict(device=device, dtype=torch.int32)
    s = types.SimpleNamespace(
        B=B, nb=nb, Lmax=Lmax, seq=torch.zeros((2, R, Lmax), **i32), beam_scores=torch.zeros(R, device=device, dtype=torch.float32),
        done=torch.zeros(B, **i32), hyp_cnt=torch.zeros(B, **i32), hyp_worst=torch.zeros(B, device=device, dtype=torch.float64),
        hyp_score=torch.zeros((B, nb), device=device, dtype=torch.float64), hyp_len=torch.zeros((B, nb), **i32),
        hyp_seq=torch.zeros((B, nb, Lmax), **i32), next_ids=torch.zeros(R, device=device, dtype=torch.int64),
        src_idx=torch.zeros(R, device=device, dtype=torch.int64),
        bans=torch.full((R, Lmax + n_bad), -1, **i32) if no_repeat_ngram_size > 0 or n_bad > 0 else None, bad_words=bad_words)
    s.st = _lib.BeamState(seq0=s.seq[0].data_ptr(), seq1=s.seq[1].data_ptr(), beam_scores=_p(s.beam_scores), done=_p(s.done),
                          hyp_cnt=_p(s.hyp_cnt), hyp_worst=_p(s.hyp_worst), hyp_score=_p(s.hyp_score), hyp_len=_p(s.hyp_len),
                          hyp_seq=_p(s.hyp_seq), next_ids=_p(s.next_ids), src_idx=_p(s.src_idx), bans=_p(s.bans), B=B, nb=nb, Lmax=Lmax,
                          V=V, eos=eos, pad=pad, no_repeat_ngram_size=no_repeat_ngram_size, early_stopping=int(bool(early_stopping)),
                          length_penalty=float(length_penalty), **bw)
    s.groups = None if groups is None else (int(groups[0]), float(groups[1]))
    return s


def beam_init(state, start_token):
    call("vacnic_beam_init", _lib.C.byref(state.st), int(start_token), _stream())


def beam_step(state, top_val, top_idx, cur_len):
    """one position of the on-device beam bookkeeping: top_val f32 / top_idx int32 [B * nb, K2] from beam_topk / lmhead_topk."""
    call("vacnic_beam_step", _lib.C.byref(state.st), _p(top_val), _p(top_idx), top_val.shape[1], int(cur_len), _stream())


def group_beam_init(state, start_token, groups=None):
    """vacnic_group_beam_init on a beam_alloc state: slot 0 of every group starts live (groups defaults to the state's own)"""
    ga = group_beam_args(groups or state.groups or (1, 0.0))
    call("vacnic_group_beam_init", _lib.C.byref(state.st), _lib.C.byref(ga), int(start_token), _stream())


def group_beam_step(state, top_val, top_idx, cur_len, groups=None, forced_token=-1, repetition_penalty=1.0, penalty_rule=None):
    """one position of group (diverse) beam search bookkeeping; forced_token / repetition_penalty / penalty_rule: those of the top-k
    call that produced top_val / top_idx (the Hamming term skips a forced position and carries the penalty's factor)."""
    ga = group_beam_args(groups or state.groups or (1, 0.0), forced_token, repetition_penalty, penalty_rule)
    call("vacnic_group_beam_step", _lib.C.byref(state.st), _lib.C.byref(ga), _p(top_val), _p(top_idx), top_val.shape[1], int(cur_len), _stream())
