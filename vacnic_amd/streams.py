"""Side HIP streams that fill the GPU's bubbles.

Measured on MI355X (profiles/r1_gemm_overhead.txt): a 256x256-tile GEMM launch carries ~10 us of launch + prologue +
epilogue time plus its store tail, during which most CUs idle, and the chain of ~3000 dependent launches of one training
step exposes all of it.  Two pieces of work are independent of the main chain and are therefore issued on their own
streams so the hardware can schedule their workgroups into those bubbles:
  * the frozen guide-BART forward (TRAIN:293-294) — needed only by the CoLaM loss at the end of the forward — and the
    frozen CLIP ViT forward; both depend only on the batch, NOT on the weights AdamW is still updating, so when the
    caller vouches for the batch (`ready` event) they start while the previous step's AdamW is running;
  * every weight-gradient GEMM + bias-gradient reduction of the backward pass — needed only by AdamW / the DDP reducer.
Side-stream work is launched through kernels.launch_on(raw stream) and every cross-stream edge is a kernels.fence():
torch (allocator, autograd engine) sees ONE stream, so no synchronisation is hidden inside torch and the step's launch
sequence, fences included, can be recorded into a launch plan (training.PlannedTrainStep).  Because the allocator only
knows the compute stream, tensors consumed on a side stream are kept alive by the keep-list until the compute stream has
joined that stream (`join_all`), NOT by Tensor.record_stream(): with recorded blocks outstanding the caching allocator polls
their events on every allocation, which cost ~14 us per torch.empty (16 ms of host time per step).  The list has one owner:
kernels._p appends every tensor handed to a kernel inside a launch_on section, so no call site keeps tensors by hand.

`raw(name)` is the one way to a side stream's handle (None when side streams are off: the caller then launches where it stands);
the torch Stream objects (`aux_stream()` ...) are for the places that need one: wait_event, torch.cuda.stream, torch collectives.
"""
import torch

from . import kernels as _K

_state = {"enabled": False, "wgrad": None, "aux": None, "vit": None, "branch": None, "keep": []}
_raw = {}                 # name -> hipStream_t (Stream.cuda_stream is a property that builds a Python int on every read)
_K._KEEP = _state["keep"]


def enable(flag=True):
    _state["enabled"] = bool(flag) and torch.cuda.is_available()
    if _state["enabled"] and _state["wgrad"] is None:
        _state["wgrad"] = torch.cuda.Stream()
        _state["aux"] = torch.cuda.Stream()
        # the two frozen towers share ONE stream (ViT first: the student needs it first): same-box A/B 65.1 vs 66.0 ms/step
        # (profiles/r3_step_ab_towers.txt) — two towers running beside each other AND beside the backward chain take more CUs away
        # from that chain than their overlap buys
        _state["vit"] = _state["aux"]
        _state["branch"] = torch.cuda.Stream()
        _raw.update((n, _state[n].cuda_stream) for n in ("wgrad", "aux", "vit", "branch"))


def raw(name):
    """raw hipStream_t of side stream 'wgrad' | 'aux' | 'vit' | 'branch' (None when side streams are off)."""
    return _raw[name] if _state["enabled"] else None


def enabled():
    return _state["enabled"]


def wgrad_stream():
    return _state["wgrad"] if _state["enabled"] else None


def pending_keep():
    """number of tensors still held for the side streams (0 right after join_all)."""
    return len(_state["keep"])


def branch_stream():
    """stream of the encoder layer's small-token branches (image / face / name streams of MFULL:647-691: a dozen GEMMs over
    20-80 tokens per sample that occupy a fraction of the GPU) — they run beside the text self-attention block of the same
    layer, forward and backward (the autograd engine replays each node on the stream of its forward)."""
    return _state["branch"] if _state["enabled"] else None


def aux_stream():
    return _state["aux"] if _state["enabled"] else None


def vit_stream():
    return _state["vit"] if _state["enabled"] else None


def release_keep():
    """drop the references held for the side streams (the caller has ordered the compute stream behind all of them)."""
    _state["keep"].clear()


def join_all(skip_wgrad=False):
    """make the current stream wait for everything issued on the side streams (before AdamW / the all-reduce tail).
    skip_wgrad: the weight-gradient stream is joined piecewise by the data-parallel reducer (one named event per gradient bucket,
    the last of them behind everything that stream was given); the keep-list then stays until release_keep()."""
    if _state["enabled"]:
        cur = _K._stream()
        for name in ("wgrad", "aux", "branch"):          # (the ViT runs on the aux stream)
            if name == "wgrad" and skip_wgrad:
                continue
            _K.fence(_raw[name], cur)
        if not skip_wgrad:
            _state["keep"].clear()
