"""autograd wrapper of the MFMA implicit-GEMM convolution (csrc/conv_mfma.hip) and its registration as the
convolution implementation of :mod:`oadg_amd.layers`.

Forward (C and K multiples of 64, else None to :mod:`oadg_amd.layers`), data gradients (stride 1 and 2) and weight
gradients run on the hand-written kernels.  ``_Conv2dMFMA.backward`` is four steps (``_incoming_grad``, ``_data_grad``,
``_weight_grad``, ``_residual_grad``) around the ``GradToken`` hand-offs; ``aten.convolution_backward`` (MIOpen) remains
for data gradients without a second weight copy (``_wt_useful`` 0) and weight gradients with C or K no multiple of 128.
"""
import collections
import ctypes
import os
import weakref

import numpy as np
import torch

from . import _lib, staging
from ._lib import check, ptr, stream_ptr

_ZEROS = {}
USE_HIP_WGRAD = 'auto'      # True / False / 'auto' (= where tools/bench_conv.py --wgrad shows a win over MIOpen)
# live HIP-event timing of the kernel launches inside bench.py's timed region: list of (start, end, flops, bytes,
# kernel name)
# (bytes = algorithmic HBM bytes of the launch: input + weights + output [+ residual], each touched once)
TIMERS = None
# restrict the event pairs to some kernel families (a set of: conv variant numbers 2 / 3 / 4 = 256-tile / 128-tile /
# streaming pointwise, 'wgrad256', 'wgrad128'): ~50 events per step instead of ~350
TIMERS_ONLY_VARIANT = None


def _t0(family):
    """the recorded start event of a launch of kernel ``family`` when bench.py times that family, else None (the untimed
    path: one global read and a comparison)"""
    if TIMERS is None:
        return None
    only = TIMERS_ONLY_VARIANT
    if not (only is None or family == only or (isinstance(only, (set, frozenset, tuple, list)) and family in only)):
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _t1(e0, flops, nbytes, name, geo):
    """the end of the launch ``_t0`` opened: one TIMERS entry"""
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    TIMERS.append((e0, e1, flops, nbytes, name, geo))


def _wgrad_cost(x16, gy16, K, R, S):
    """(FLOP, algorithmic bytes) of a weight gradient: x and dy read once, dW (fp32) written once; the split partials are
    implementation traffic"""
    N, C, H, W = x16.shape
    P = N * gy16.shape[2] * gy16.shape[3]
    return 2.0 * P * K * C * R * S, 2.0 * (N * H * W * C + P * K) + 4.0 * K * C * R * S


def _wgrad_begin(x16, gy16, K, R, S):
    """what the single-layer weight-gradient launches start with: (workspace bytes, workspace, start event or None,
    kernel name when timed)"""
    L = _lib.lib()
    N, C = x16.shape[0], x16.shape[1]
    Ho, Wo = gy16.shape[2], gy16.shape[3]
    nbytes = L.oadg_conv2d_wgrad_workspace_bytes(N, Ho, Wo, C, K, R, S)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x16.device)
    e0 = name = None
    if TIMERS is not None:
        v = L.oadg_conv2d_wgrad_variant(N, Ho, Wo, C, K, R, S)
        e0 = _t0('wgrad256' if v == 256 else 'wgrad128')
        name = 'conv_wgrad256_kernel' if v == 256 else 'conv_wgrad_kernel<%d>' % v
    return nbytes, ws, e0, name


def _wgrad_end(e0, name, x16, gy16, K, R, S, stride):
    N, C, H, W = x16.shape
    _t1(e0, *_wgrad_cost(x16, gy16, K, R, S), name, (N, H, W, C, K, R, stride, False, False, 1))


def _zeros(device):
    z = _ZEROS.get(device)
    if z is None:
        z = _ZEROS[device] = torch.zeros(64, dtype=torch.uint8, device=device)
    return z


def supported(x, weight, stride, padding, dilation):
    K, C, R, S = weight.shape
    return (x.is_cuda and x.dim() == 4 and C % 64 == 0 and K % 64 == 0 and stride[0] == stride[1] and
            padding[0] == padding[1] and dilation[0] == dilation[1] and R == S)


# ---- deferred column sums -------------------------------------------------------------------------------------------
# A data-gradient launch leaves the producer's bias gradient as per-tile partial sums; reducing them is a 6 us launch
# per layer (48 per step).  Nothing on the device needs the reduced vector before the optimizer (it only travels up the
# graph to AccumulateGrad, and into the BN-fold chain rule of _PrepWeights.backward as ONE term of dgamma), so inside
# TrainEngine's backward the reductions are collected and run as one launch at the end (or before a gradient bucket is
# packed): DEFER_COLSUM.  A pending vector is never read early: the producer resolves it on the spot unless its
# prepared weights are used exactly once this step (shared convolutions get their bias gradients SUMMED by autograd),
# and _PrepWeights.backward leaves dgamma raw for the deferred launch to finish with the same expression.
DEFER_COLSUM = False
DEFER_WGRAD = False         # the same for the small layers' weight gradients ("deferred, grouped weight gradients" below)
_PENDING = []
_STEP = 0                 # training-step counter: a bank entry counts the forward uses of its parameters per step


def begin_step(defer):
    """TrainEngine: a new step starts; ``defer``: collect the column-sum reductions and the small layers' weight
    gradients of its backward pass"""
    global _STEP, DEFER_COLSUM, DEFER_WGRAD
    _STEP += 1
    from . import hip_ops
    hip_ops.sink_reset()
    DEFER_COLSUM = bool(defer) and os.environ.get('OADG_DEFER_COLSUM', '1') == '1'
    DEFER_WGRAD = bool(defer) and os.environ.get('OADG_DEFER_WGRAD', '1') == '1'


def end_backward():
    """TrainEngine: the backward pass has been enqueued - run what was deferred, stop deferring"""
    global DEFER_COLSUM, DEFER_WGRAD
    DEFER_COLSUM = DEFER_WGRAD = False
    return flush_deferred(final=True)


def flush_deferred(final=False):
    """everything a backward pass has deferred so far, on the current stream: the grouped weight gradients first (their
    consumer leaves raw BN-scale dot products that the column-sum launch finishes), then the column sums.  Called at the
    end of the backward pass (``final``) and before a data-parallel gradient bucket is packed."""
    if final and _SHARED_OPEN:
        _close_shared_leftovers()
    n = flush_wgrads()
    return n + flush_colsums()


def _close_shared_leftovers():
    """a shared weight some of whose expected uses never reached _PrepWeights.backward (a level without a gradient): the
    jobs that did arrive returned no gradient, so their sum is added to the parameter's gradient here"""
    for ent in list(_SHARED_OPEN):
        if not ent.shared:
            continue
        w = ent.src[0]
        R, S = ent.shared[0].R, ent.shared[0].S
        wd = w.detach()
        krsc = int(R * S > 1 and not wd.is_contiguous() and wd.is_contiguous(memory_format=torch.channels_last))
        dw = torch.empty_like(wd)
        _enqueue_shared(ent, _Consumer(gbias=None, w=wd, scale=None, mean=None, var=None, eps=0.0, flags=krsc, dw=dw,
                                       dgamma=None))
        flush_wgrads()
        # This runs AFTER the backward pass: AccumulateGrad and its hooks are bypassed.  With no gradient on the parameter
        # yet (the normal case: none of the arrived uses returned one) a data-parallel reducer still sees it - its bucket
        # has a pending member and is packed by FlatGradReducer.finish(), which runs after end_backward().  A parameter
        # that ALREADY holds a gradient may sit in a bucket whose all-reduce is in flight: adding to it now would be lost.
        from . import hip_ops
        if w.grad is None:
            w.grad = dw
        elif hip_ops.GRAD_SINK is not None:
            raise RuntimeError('a shared convolution weight received part of its gradient through autograd and part of it '
                               'after the backward pass while a gradient reducer is active: set OADG_WGRAD_SHARED=0')
        else:
            w.grad.add_(dw)
    _SHARED_OPEN.clear()


class _PendingColsum:
    __slots__ = ('part', 'out', 'fix', 'done', 'targets')

    def __init__(self, part, out):
        # ``out`` / the tensors of ``fix`` are ALIASES (detach()) of the vectors that travel up the graph: they keep the
        # storage alive without adding a reference to the travelling tensor itself - AccumulateGrad only adopts a
        # gradient it holds the last reference to, otherwise it copies it (here: before the flush has written it)
        self.part, self.out, self.fix, self.done = part, out.detach(), None, False
        self.targets = []           # (parameter, alias): where the vector is expected to end up as .grad


def _colsum(part, K):
    """the reduced column sums of ``part`` [rows][K] - now, or (DEFER_COLSUM) as a pending vector of flush_colsums()"""
    cs = torch.empty((K,), dtype=torch.float32, device=part.device)
    if DEFER_COLSUM:
        ent = _PendingColsum(part, cs)
        cs._oadg_pending = ent
        _PENDING.append(ent)
    else:
        check(_lib.lib().oadg_colsum_reduce(ptr(part), part.shape[0], K, ptr(cs), stream_ptr()), 'oadg_colsum_reduce')
    return cs


def pending_colsum(t):
    ent = getattr(t, '_oadg_pending', None) if t is not None else None
    return ent if (ent is not None and not ent.done) else None


def resolve_colsum(t):
    """reduce a pending vector now (its consumer is about to read it on the device)"""
    ent = pending_colsum(t)
    if ent is not None:
        check(_lib.lib().oadg_colsum_reduce(ptr(ent.part), ent.part.shape[0], ent.out.shape[0], ptr(ent.out),
                                            stream_ptr()), 'oadg_colsum_reduce')
        ent.done, ent.part = True, None
        _PENDING.remove(ent)
    return t


def flush_colsums():
    """all pending reductions (and the dgamma terms that wait for them) in one launch on the current stream"""
    global _PENDING
    pend, _PENDING = _PENDING, []
    if not pend:
        return 0
    dev = pend[0].out.device
    tab = np.zeros(len(pend), dtype=_lib.COLSUM_JOB)
    blocks = 0
    for i, e in enumerate(pend):
        K = e.out.shape[0]
        r = tab[i]
        r['part'], r['out'], r['rows'], r['K'], r['first_block'] = e.part.data_ptr(), e.out.data_ptr(), e.part.shape[0], K, blocks
        if e.fix is not None:
            dg, mean, var, eps = e.fix
            r['dgamma'], r['mean'], r['var'], r['eps'] = dg.data_ptr(), mean.data_ptr(), var.data_ptr(), eps
        blocks += (K + 15) // 16
    tdev = _STAGE.upload(tab, dev)         # a few flushes per step at most (one per gradient bucket)
    check(_lib.lib().oadg_colsum_reduce_multi(ptr(tdev), len(pend), blocks, stream_ptr()), 'oadg_colsum_reduce_multi')
    for e in pend:
        _refresh_copied_grads(e.targets)
        e.done, e.part, e.fix, e.targets = True, None, None, []
    return len(pend)


def _refresh_copied_grads(targets):
    """[(parameter, alias of the tensor a deferred launch has just filled)]: AccumulateGrad adopts a gradient it holds the
    last reference to - then .grad IS that tensor.  Had it copied instead (a tensor hook, an extra reference), the copy was
    taken before the launch: refresh it."""
    for prm, alias in targets:
        g = prm.grad
        if g is not None and g.data_ptr() != alias.data_ptr() and g.shape == alias.shape:
            g.copy_(alias)


# ---- deferred, grouped weight gradients ---------------------------------------------------------------------------------
# The weight gradient of a layer is consumed by nobody but AccumulateGrad (through _PrepWeights.backward).  The small maps
# of the backbone / neck cannot fill the chip with long workgroups on their own (csrc conv_wgrad256_multi_kernel), so
# inside TrainEngine's backward their launches are collected and issued in groups: one weight-gradient launch + one
# launch of the partial-sum / BN-fold consumer per group.  dW / dgamma travel up the graph as tensors that the group's
# launches fill later - the same arrangement, with the same aliasing rules, as the deferred column sums above.
WGRAD_SMALL =int(os.environ.get('OADG_WGRAD_SMALL', 40000))        # weight tiles x K-tiles below which a layer is deferred
# ... and the sum at which a group is launched.  Round 5: 65536 -> 196608 - with lists of several rounds (the planner's dispatch
# replay) a larger group packs better and pays fewer launch tails: 27.3 -> 27.0 ms per step (131072: 27.1, 262144: 27.5 - a
# list of more than three rounds is not planned), R101-DC5 18.4 -> 18.0
WGRAD_GROUP = int(os.environ.get('OADG_WGRAD_GROUP', 196608))
_WQ = []
_WQ_WORK = 0
SHARED_GROUP = os.environ.get('OADG_WGRAD_SHARED', '1') == '1'      # the uses of a shared weight as ONE grouped launch
_SHARED_OPEN = set()        # bank entries holding jobs of a shared weight whose last use has not arrived yet


# host table -> device memory without a blocking copy (weight-gradient jobs, BN-fold consumer jobs, column-sum jobs): a slot
# whose last copy is still queued is stepped around, not waited for
_STAGE = staging.Ring(16, 64 * ctypes.sizeof(_lib.WgradJob), grow_when_busy=True)


def wgrad_work(N, Ho, Wo, C, K, R, S):
    """weight tiles x K-tiles of a weight-gradient problem on the 256-tile kernel (0: not that kernel's shape)"""
    if K % 256 or C % 256:
        return 0
    return (K // 256) * (C // 256) * R * S * ((N * Ho * Wo + 63) // 64)


# LDS limits of the two consumer kernels of csrc/conv_mfma.hip, in their own units:
MULTI_CONSUMER_LDS_FLOATS = 36000       # oadg_prep_conv_weights_bwd_parts_multi: max_crs, one C * R * S row of floats
PARTS_CONSUMER_LDS_BYTES = 12000        # oadg_prep_conv_weights_bwd_parts: the bytes of one C * R * S row (it keeps five)


# the operands of one job of the consumer launch (BN-fold chain rule, layout change, sum over the splits): csrc
# oadg_prep_bwd_job; ``dw`` / ``dgamma`` are aliases of the tensors that went up the graph
_Consumer = collections.namedtuple('_Consumer', 'gbias w scale mean var eps flags dw dgamma')


class _WgradJob:
    """one deferred weight gradient.  Either its operands ``x`` / ``gy`` (kept alive; launched with the group), or - a
    single-layer launch has run already - its split partials ``parts`` / ``splits``: then only the consumer waits for the
    group's consumer launch.  ``consumer`` / ``targets``: set by _PrepWeights.backward; ``consumer`` stays None on a
    member of a shared-weight set."""
    __slots__ = ('x', 'gy', 'parts', 'splits', 'C', 'K', 'R', 'S', 'stride', 'pad', 'dil', 'work', 'consumer', 'targets',
                 'members')

    def __init__(self, C, K, R, S, x=None, gy=None, stride=1, pad=0, dil=1, parts=None, splits=0):
        self.x, self.gy, self.parts, self.splits = x, gy, parts, int(splits)
        self.C, self.K, self.R, self.S, self.stride, self.pad, self.dil = C, K, R, S, stride, pad, dil
        self.work = wgrad_work(x.shape[0], gy.shape[2], gy.shape[3], C, K, R, S) if x is not None else 0
        self.consumer, self.targets = None, []      # targets: (parameter, alias) - where dW / dgamma should end up as .grad
        self.members = 1            # > 1: the leader of a shared-weight set - the next members - 1 jobs of the queue are uses
                                    # of the same weight whose partials its consumer sums with its own


def _enqueue(job):
    global _WQ_WORK
    _WQ.append(job)
    _WQ_WORK += job.work


def _enqueue_shared(ent, consumer):
    """the jobs waiting on bank entry ``ent`` as one shared-weight set: the first leads with ``consumer``, all enter the
    queue side by side"""
    jobs, ent.shared = ent.shared, []
    _SHARED_OPEN.discard(ent)
    jobs[0].consumer, jobs[0].members = consumer, len(jobs)
    for j in jobs:
        _enqueue(j)


_GROUP_TRACE = {} if os.environ.get('OADG_BENCH_DIAG_CONV') == '1' else None


def wgrad_multi(jobs, target_blocks=256):
    """[(x16, gy16, K, R, S, stride, pad, dil)] -> (workspace, [(part pointer, splits)] per job): the weight gradients of
    several layers as fp32 split partials from ONE launch (csrc oadg_conv2d_wgrad_multi)"""
    L = _lib.lib()
    tab = np.zeros(len(jobs), dtype=_lib.WGRAD_JOB)
    dev = jobs[0][0].device
    for r, (x16, gy16, K, R, S, stride, pad, dil) in zip(tab, jobs):
        N, C, H, W = x16.shape
        r['x'], r['dy'] = x16.data_ptr(), gy16.data_ptr()
        r['N'], r['H'], r['W'], r['C'], r['K'], r['R'], r['S'] = N, H, W, C, K, R, S
        r['stride'], r['pad'], r['dil'] = stride, pad, dil
    xcd_first = (ctypes.c_int * 9)()        # the list's eight XCD slices (equal work)
    total = L.oadg_conv2d_wgrad_multi_plan(tab.ctypes.data_as(ctypes.c_void_p), len(jobs), int(target_blocks), xcd_first)
    if total <= 0:
        raise RuntimeError(f'oadg_conv2d_wgrad_multi_plan failed (code {-total})')
    sizes = [int(r['splits']) * int(r['K']) * int(r['R']) * int(r['S']) * int(r['C']) * 4 for r in tab]
    ws = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
    off, parts = 0, []
    for r, (x16, gy16, *_), sz in zip(tab, jobs, sizes):
        assert gy16.shape[2] == r['Ho'] and gy16.shape[3] == r['Wo'], 'dy does not have the convolution\'s output extent'
        r['part'] = ws.data_ptr() + off
        parts.append((ws.data_ptr() + off, int(r['splits'])))
        off += sz
    e0 = _t0('wgrad256')
    tdev = _STAGE.upload(tab, dev)
    check(L.oadg_conv2d_wgrad_multi(ptr(tdev), len(jobs), int(total), xcd_first, ptr(_zeros(dev)), stream_ptr()),
          'oadg_conv2d_wgrad_multi')
    if e0 is not None:
        costs = [_wgrad_cost(*j[:5]) for j in jobs]
        _t1(e0, sum(c[0] for c in costs), sum(c[1] for c in costs), 'conv_wgrad256_multi_kernel',
            (len(jobs), 0, 0, 0, 0, 0, 0, False, False, 1))
        if _GROUP_TRACE is not None:
            key = tuple((int(r['N']), int(r['H']), int(r['W']), int(r['C']), int(r['K']), int(r['R']), int(r['splits'])) for r in tab)
            if key not in _GROUP_TRACE:      # bench.py OADG_BENCH_DIAG_CONV: what each grouped launch is made of
                _GROUP_TRACE[key] = int(total)
    return ws, parts


def flush_wgrads():
    """launch the deferred weight gradients collected so far as ONE group (+ one launch of their consumer), on the current
    stream (a second stream for them was measured again in round 6 and not kept - HISTORY.md, the table of round 6;
    R50-FPN with every group there: 26.84 against 26.82 ms per step)"""
    global _WQ, _WQ_WORK
    jobs, _WQ, _WQ_WORK = _WQ, [], 0
    if not jobs:
        return 0
    L = _lib.lib()
    dev = next(j.consumer.w.device for j in jobs if j.consumer is not None)
    launch = [j for j in jobs if j.parts is None]
    ws, parts = wgrad_multi([(j.x, j.gy, j.K, j.R, j.S, j.stride, j.pad, j.dil) for j in launch]) if launch else (None, [])
    parts = iter(parts)
    parts = [next(parts) if j.parts is None else (j.parts.data_ptr(), j.splits) for j in jobs]
    # consumer jobs: one per queue entry that has consumer operands; the leader of a shared-weight set takes the partials of
    # its members too (they follow it in the queue, hence in the workspace: one array of sum(splits) tiles)
    cons = []
    for i, j in enumerate(jobs):
        if j.consumer is None:
            continue
        pp, splits = parts[i]
        for m_ in jobs[i + 1:i + j.members]:
            assert m_.consumer is None and (m_.C, m_.K, m_.R, m_.S) == (j.C, j.K, j.R, j.S)
        splits += sum(sp for _, sp in parts[i + 1:i + j.members])
        cons.append((j, pp, splits))
    tab = np.zeros(len(cons), dtype=_lib.PREP_BWD_JOB)
    first, max_crs = 0, 0
    p_ = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    for r, (j, pp, splits) in zip(tab, cons):
        c = j.consumer
        r['part'], r['gbias'], r['w'], r['scale'], r['mean'], r['var'] = pp, p_(c.gbias), p_(c.w), p_(c.scale), p_(c.mean), p_(c.var)
        r['dw'], r['dgamma'], r['eps'], r['splits'] = p_(c.dw), p_(c.dgamma), c.eps, splits
        r['K'], r['C'], r['R'], r['S'], r['w_krsc'], r['first_block'] = j.K, j.C, j.R, j.S, c.flags, first
        first += j.K
        max_crs = max(max_crs, j.C * j.R * j.S)
    tdev = _STAGE.upload(tab, dev)
    check(L.oadg_prep_conv_weights_bwd_parts_multi(ptr(tdev), len(cons), first, max_crs, stream_ptr()),
          'oadg_prep_conv_weights_bwd_parts_multi')
    for j in jobs:
        _refresh_copied_grads(j.targets)
        j.x = j.gy = j.parts = j.consumer = None
        j.targets = []
    return len(jobs)


TOPDOWN_FUSED = os.environ.get('OADG_TOPDOWN_FUSED', '1') == '1'


def topdown_ok(x, K, top):
    """may ``conv1x1(x) + nearest_upsample_2x(top)`` run as ONE launch (the FPN top-down add in the lateral convolution's
    epilogue: csrc ConvArgs.res_up)?  The streaming pointwise kernel, even map sizes, ``top`` exactly half the size."""
    if not (on_path(x) and TOPDOWN_FUSED and top.is_cuda and x.dim() == 4 and top.dtype == torch.bfloat16):
        return False
    N, C, H, W = x.shape
    if tuple(top.shape) != (N, K, H // 2, W // 2) or H & 1 or W & 1 or H < 2 or W < 2 or N * H * W >= 1 << 31:
        return False
    return _lib.lib().oadg_conv2d_auto_variant(N, H, W, C, K, 1, 1, 1, 0, 1) == 4


def conv_forward(x, w, bias, residual, stride, pad, dil, relu, variant=0, mask=None, want_colsum=False, mask_bits=None,
                 bits_out=None, res_up=False):
    """x [N,C,H,W] bf16 channels_last, w [K,C,R,S] bf16 channels_last -> y [N,K,Ho,Wo] bf16 channels_last.
    ``mask`` (same shape as y): y *= (mask > 0); ``want_colsum``: also return sum of the stored y over (N,H,W)
    (fp32 [K], deterministic) - the two together are the backward of a producer's bias + ReLU epilogue.
    ``mask_bits`` (uint8 [rows * K / 8]): the same mask, one bit per element (1/16 of the bytes); ``bits_out``: a uint8
    tensor of that size which receives (y > 0) - what a later data-gradient launch passes as ``mask_bits``."""
    L = _lib.lib()
    N, C, H, W = x.shape
    K, _, R, S = w.shape
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    y = torch.empty((N, K, Ho, Wo), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    # the kernel is resolved here (geometry, then operands) so that the column-sum rows and the launch agree
    variant = int(variant) or L.oadg_conv2d_auto_variant(N, H, W, C, K, R, S, stride, pad, dil)
    if variant == 4 and (mask is not None or (mask_bits is not None and bits_out is not None)):
        variant = 3                                    # the streaming pointwise kernel takes mask BITS, or writes them
    e0 = _t0(int(variant))                             # bench.py: only the dominant kernel family carries events
    part = None
    if want_colsum:
        rows = L.oadg_conv2d_pixel_tiles(N, H, W, C, K, R, S, stride, pad, dil, int(variant))
        part = torch.empty((rows, K), dtype=torch.float32, device=x.device)
    check(L.oadg_conv2d_nhwc_bf16_ex(ptr(x), ptr(w), ptr(bias), ptr(residual), ptr(y), ptr(_zeros(x.device)), N,
                                     H, W, C, K, R, S, stride, pad, dil, int(bool(relu)) | (2 if res_up else 0), int(variant), ptr(mask),
                                     ptr(part), ptr(mask_bits), ptr(bits_out), stream_ptr()),
          'oadg_conv2d_nhwc_bf16')
    if e0 is not None:
        _t1(e0, 2.0 * N * Ho * Wo * K * C * R * S,
            2.0 * (N * H * W * C + K * C * R * S +
                   N * Ho * Wo * K * (1 + (residual is not None) * (0.25 if res_up else 1) + (mask is not None)) +
                   N * Ho * Wo * K / 16.0 * ((mask_bits is not None) + (bits_out is not None))),
            kernel_name(variant, C, K, R, S, stride, pad, residual is not None, mask is not None, mask_bits is not None,
                        bits_out is not None),
            (N, H, W, C, K, R, stride, residual is not None, mask is not None, dil))
    if want_colsum:
        return y, _colsum(part, K)
    return y


def kernel_name(v, C, K, R, S, stride, pad, res, mask, bits_in, bits_out, scatter=False):
    """the instantiation csrc conv_launch runs for variant ``v`` with these operands, spelt as rocprofv3 prints it (minus
    namespace and argument list): bench.py keys its live timers and the committed PMC summaries on this string"""
    b = lambda f: 'true' if f else 'false'  # noqa: E731
    post = res or mask or bits_in
    if v == 2:
        return 'conv_igemm256_kernel<%s, %d>' % (b(post), 2 if K % 256 == 0 else 1)      # (256 x 128 tiles for K = 128)
    if v == 4:
        return 'conv_pw_stream_kernel<%d, %s, %s, %s>' % (C, b(res), b(bits_in), b(bits_out))
    pw = v == 3 and R == 1 and S == 1 and stride == 1 and pad == 0 and not scatter
    return 'conv_igemm_kernel<%d, %s, %d, %s>' % (128 if K % 128 == 0 else 64, b(post), 1 if v == 3 else 2, b(pw))


_S2_CLASSES = ((0, 0, 1, 1, 0), (0, 1, 1, 2, 1), (1, 0, 2, 1, 3), (1, 1, 2, 2, 5))    # ph, pw, taps_h, taps_w, block offset
S2_ONE_LAUNCH = True        # the parity classes of a stride-2 data gradient in one launch (False: one scatter launch per class)


def conv_dgrad_s2(gy, wt, xshape, R, mask=None, want_colsum=False, mask_bits=None, accumulate=None):
    """dx of a stride-2 convolution (3x3 / pad 1 or 1x1 / pad 0) as one stride-1 convolution over dy per output parity
    class, each written on its strided grid of dx (csrc oadg_conv2d_nhwc_bf16_scatter; ``wt`` = the class filters from
    ``_PrepWeights`` mode 2).  ``mask``: ReLU-backward mask (the convolution's input), ``want_colsum``: also return the
    column sums of the masked dx (the producer's bias gradient) - the same epilogue fusions as the stride-1 path."""
    L = _lib.lib()
    N, C, H, W = xshape
    K, Ho, Wo = gy.shape[1], gy.shape[2], gy.shape[3]
    classes = _S2_CLASSES if R == 3 else _S2_CLASSES[:1]
    if accumulate is not None:
        # 1x1 / stride 2 only: dx += on the even rows / columns of an existing gradient (bf16 NHWC), in place - the
        # launch reads its residual operand and writes its output at the same addresses
        assert R == 1 and accumulate.shape == (N, C, H, W) and accumulate.dtype == torch.bfloat16 and \
            accumulate.is_contiguous(memory_format=torch.channels_last) and mask is None and mask_bits is None
        gx = accumulate
    else:
        gx = torch.empty((N, C, H, W), dtype=torch.bfloat16, device=gy.device, memory_format=torch.channels_last)
        if R == 1:
            gx.zero_()                   # odd rows / columns receive no gradient
    geo = []
    for ph, pw, th, tw, off in classes:
        ha, wa = (H - ph + 1) // 2, (W - pw + 1) // 2
        if ha > 0 and wa > 0:
            geo.append((ph, pw, th, tw, off, ha, wa, (N * ha * wa + 127) // 128))
    part = torch.empty((sum(g[-1] for g in geo), C), dtype=torch.float32, device=gy.device) if want_colsum else None
    row = 0
    e0 = _t0(3)
    if S2_ONE_LAUNCH:
        # all classes in one launch (csrc conv_igemm_s2_kernel): dy from HBM once, one launch ramp
        check(L.oadg_conv2d_dgrad_s2_nhwc_bf16(ptr(gy), ptr(wt), ptr(accumulate), ptr(gx), ptr(_zeros(gy.device)), N, Ho, Wo, K, C,
                                               R, H, W, ptr(mask), ptr(part), ptr(mask_bits), stream_ptr()),
              'oadg_conv2d_dgrad_s2_nhwc_bf16')
        geo_loop = ()
    else:
        geo_loop = geo
    for ph, pw, th, tw, off, ha, wa, tiles in geo_loop:
        wptr = ctypes.c_void_p(wt.data_ptr() + off * C * K * 2)
        pptr = ctypes.c_void_p(part.data_ptr() + row * C * 4) if part is not None else None
        check(L.oadg_conv2d_nhwc_bf16_scatter(ptr(gy), wptr, None, ptr(accumulate), ptr(gx), ptr(_zeros(gy.device)), N, Ho, Wo, K, C,
                                              th, tw, 0, 1, 0, ha, wa, H, W, 2, 2, ph, pw, ptr(mask), pptr,
                                              ptr(mask_bits), stream_ptr()), 'oadg_conv2d_nhwc_bf16_scatter')
        row += tiles
    if e0 is not None:
        # the class launches of one stride-2 data gradient as ONE entry: 2 * (output pixels of the forward conv) * K * C
        # * R * S FLOP (no zero-inserted dy), dy + the class filters read, dx (+ residual / mask) touched once
        post = accumulate is not None or mask is not None or mask_bits is not None
        _t1(e0, 2.0 * N * Ho * Wo * K * C * R * R,
            2.0 * (N * Ho * Wo * K + K * C * R * R + N * H * W * C * (1 + (accumulate is not None) + (mask is not None)))
            + N * H * W * C / 8.0 * (mask_bits is not None),
            ('conv_igemm_s2_kernel<%d, %s>' % (128 if C % 128 == 0 else 64, 'true' if post else 'false')
             if S2_ONE_LAUNCH else
             kernel_name(3, K, C, 2, 2, 1, 0, accumulate is not None, mask is not None, mask_bits is not None, False,
                         scatter=True)) + ' x%d (stride-2 dgrad classes)' % len(geo),
            (N, Ho, Wo, K, C, R, 2, accumulate is not None, mask is not None, 1))
    if want_colsum:
        return gx, _colsum(part, C)
    return gx


def conv_wgrad(x16, gy16, K, R, S, stride, pad, dil):
    """dW [K,C,R,S] (fp32, channels_last strides) of y = conv(x, W): csrc/conv_mfma.hip conv_wgrad_kernel."""
    N, C, H, W = x16.shape
    dw = torch.empty((K, R, S, C), dtype=torch.float32, device=x16.device)
    nbytes, ws, e0, name = _wgrad_begin(x16, gy16, K, R, S)
    check(_lib.lib().oadg_conv2d_wgrad_nhwc_bf16(ptr(x16), ptr(gy16), ptr(dw), ptr(_zeros(x16.device)), ptr(ws), nbytes, N,
                                                 H, W, C, K, R, S, stride, pad, dil, stream_ptr()),
          'oadg_conv2d_wgrad_nhwc_bf16')
    if e0 is not None:
        _wgrad_end(e0, name + '+reduce', x16, gy16, K, R, S, stride)
    return dw.permute(0, 3, 1, 2)


def conv_wgrad_parts(x16, gy16, K, R, S, stride, pad, dil):
    """(workspace, splits): the weight gradient of y = conv(x, W) as fp32 split partials [splits][K][R*S][C]; summed
    (with the BN-fold chain rule) by _PrepWeights.backward through oadg_prep_conv_weights_bwd_parts."""
    N, C, H, W = x16.shape
    splits = ctypes.c_int(0)
    nbytes, ws, e0, name = _wgrad_begin(x16, gy16, K, R, S)
    check(_lib.lib().oadg_conv2d_wgrad_parts_nhwc_bf16(ptr(x16), ptr(gy16), ptr(_zeros(x16.device)), ptr(ws), nbytes, N, H,
                                                       W, C, K, R, S, stride, pad, dil, ctypes.byref(splits), stream_ptr()),
          'oadg_conv2d_wgrad_parts_nhwc_bf16')
    if e0 is not None:
        _wgrad_end(e0, name, x16, gy16, K, R, S, stride)
    return ws, splits.value


class WeightGradToken:
    """Hand-off of a weight gradient from the convolution's backward to the backward of its weight preparation
    (one prepared weight <-> one convolution call; weights used by several calls, e.g. the RPN conv shared by the
    pyramid levels, take the reduced path because autograd has to add their gradients)."""
    __slots__ = ('uses', 'parts', 'deferrable', 'entry')

    def __init__(self):
        self.uses, self.parts = 0, None
        self.deferrable = False      # the gradients of this preparation go straight to AccumulateGrad of bank parameters
        self.entry = None            # the bank entry of the prepared weight (shared-weight groups, _PrepWeights.backward)


_ZERO_SCALARS = {}


def _dummy_grad(like):
    key = (like.device, like.dtype)
    z = _ZERO_SCALARS.get(key)
    if z is None:
        z = _ZERO_SCALARS[key] = torch.zeros((), dtype=like.dtype, device=like.device)
    return z.expand(like.shape)


def _hip_wgrad(K, C):
    """use the csrc weight-gradient kernels?  With the per-shape kernel / split choice of conv_mfma.hip they match or
    beat MIOpen's igemm_wrw on every layer with K and C multiples of 128 (tools/bench_conv.py --wgrad: 1.0-1.6x)."""
    return bool(USE_HIP_WGRAD) and K % 128 == 0 and C % 128 == 0        # ('auto' = wherever the kernels apply)


def _group_sized(deferrable, x16, Ho, Wo, K, C, R, S):
    """is this layer's weight gradient small enough to ride in a group (flush_wgrads)?  ONE rule for _Conv2dMFMA.forward,
    which counts the jobs a shared weight will receive, and _Conv2dMFMA.backward, which creates them: if the two disagreed,
    every use of the shared weight would end in _close_shared_leftovers."""
    return deferrable and C * R * S <= MULTI_CONSUMER_LDS_FLOATS and x16.numel() < 2 ** 32 and _hip_wgrad(K, C) and \
        0 < wgrad_work(x16.shape[0], Ho, Wo, C, K, R, S) < WGRAD_SMALL


def _sole_use(ent, leaf, no_grad_yet=True):
    """do the gradients of this weight preparation go, as they are, to AccumulateGrad (``leaf``) of parameters used ONCE in
    this step (bank entry ``ent``) that hold no gradient yet?  Only then may they be filled in later: a shared
    convolution's gradients, or a second micro-batch's, are summed as they arrive."""
    return leaf and ent is not None and ent.step == _STEP and ent.count == 1 and \
        (not no_grad_yet or all(t.grad is None for t in ent.src))


def _nhwc_bf16(t):
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def relu_bias_bwd(gy, y, want_bias):
    """(g, dbias): g = bf16(gy) * (y > 0) (``y`` None: no mask) and dbias = g.sum over (N,H,W), in one pass over gy
    (csrc/eltwise.hip).  gy: fp32 or bf16 [N,K,H,W] with channels_last strides."""
    N, K, H, W = gy.shape
    f32 = gy.dtype == torch.float32
    write = f32 or y is not None
    L = _lib.lib()
    M = N * H * W
    g = torch.empty((N, K, H, W), dtype=torch.bfloat16, device=gy.device,
                    memory_format=torch.channels_last) if write else None
    nbytes = L.oadg_relu_bias_bwd_workspace_bytes(M, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gy.device)
    db = torch.empty((K,), dtype=torch.float32, device=gy.device)
    check(L.oadg_relu_bias_bwd(ptr(gy), int(f32), ptr(y), ptr(g), ptr(db), ptr(ws), nbytes, M, K, stream_ptr()),
          'oadg_relu_bias_bwd')
    return (g if write else gy), (db if want_bias else None)


def _wgrad_dest(ctx, w, K, has_bn):
    """(dW, dgamma) output tensors of a _PrepWeights.backward: the parameters' slices of the data-parallel reducer's flat
    bucket (hip_ops.grad_dest) when this is the parameters' only use of the step and they hold no gradient yet - then
    AccumulateGrad adopts them and the reducer packs nothing - else new tensors"""
    from . import hip_ops
    ent = ctx.entry
    # (no_grad_yet=False: whether the parameters hold a gradient is not asked here - with it, a second micro-batch would
    #  take other tensors than it does today)
    if hip_ops.GRAD_SINK is not None and _sole_use(ent, ctx.leaf_inputs, no_grad_yet=False) and \
            ent.src[0].dtype == torch.float32 and ent.src[0].stride() == w.stride():
        dw = hip_ops.grad_dest(ent.src[0], w)
        dgamma = None
        if has_bn:
            g = ent.src[1]
            dgamma = hip_ops.grad_dest(g) if (g.dtype == torch.float32 and g.is_contiguous()) else \
                torch.empty((K,), dtype=torch.float32, device=w.device)
        return dw, dgamma
    return torch.empty_like(w), (torch.empty((K,), dtype=torch.float32, device=w.device) if has_bn else None)


def _attach_consumer(job, ctx, gbias, w, scale, mean, var, eps, flags, has_bn, record_targets):
    """give ``job`` its consumer operands, writing to the (dW, dgamma) tensors of _wgrad_dest, which are returned;
    ``record_targets``: remember the parameters these tensors should end up on as .grad (flush_wgrads checks that)"""
    dw, dgamma = _wgrad_dest(ctx, w, w.shape[0], has_bn)
    c = job.consumer = _Consumer(gbias, w, scale, mean, var, eps, flags, dw.detach(),
                                 dgamma.detach() if dgamma is not None else None)
    if record_targets:
        job.targets.append((ctx.entry.src[0], c.dw))
        if dgamma is not None:
            job.targets.append((ctx.entry.src[1], c.dgamma))
    return dw, dgamma


class _PrepWeights(torch.autograd.Function):
    """(w fp32 [K,C,R,S], optional eval-mode BN, optional bias) -> (wf bf16 KRSC, bias fp32, wt bf16 for dgrad):
    one launch (csrc/conv_mfma.hip prep_weights_kernel) instead of the ~10 element-wise ops of the unfused fold
    and casts; the backward is one launch as well."""

    @staticmethod
    def forward(ctx, w, gamma, beta, mean, var, eps, bias_in, want_wt, wtoken=None, entry=None):
        L = _lib.lib()
        K, C, R, S = w.shape
        leaf = all(t is None or t.grad_fn is None for t in (w, gamma, beta, bias_in))
        w = w.detach() if w.dtype == torch.float32 else w.detach().float()      # (host time: ~60 layers per step)
        # a torch.channels_last parameter ([K][R][S][C] in memory) is read - and its gradient written - in place: no
        # re-layout copy forward, no stride-fixing clone in AccumulateGrad
        krsc = int(R * S > 1 and not w.is_contiguous() and w.is_contiguous(memory_format=torch.channels_last))
        if not krsc:
            w = w.contiguous()
        want_wt = int(want_wt)         # 0 none, 1 flipped / transposed copy (stride-1 dgrad), 2 stride-2 parity classes
        f = lambda t: None if t is None else (t.detach() if (t.dtype == torch.float32 and t.is_contiguous())  # noqa: E731
                                              else t.detach().float().contiguous())
        if entry is not None and entry.valid:
            # prepared by refresh_prepared() right after the last optimizer step (or by the previous forward pass with the
            # parameters unchanged since): nothing to launch
            wf, wt, bias, scale, m_, v_ = entry.wf, entry.wt, entry.bias, entry.scale, entry.mean, entry.var
        else:
            dev = w.device
            wf = torch.empty((K, C, R, S), dtype=torch.bfloat16, device=dev, memory_format=torch.channels_last)
            wt = torch.empty((C, K, R, S), dtype=torch.bfloat16, device=dev,
                             memory_format=torch.channels_last) if want_wt else None
            has_bias = gamma is not None or bias_in is not None
            bias = torch.empty((K,), dtype=torch.float32, device=dev) if has_bias else None
            scale = torch.empty((K,), dtype=torch.float32, device=dev) if gamma is not None else None
            g_, b_, m_, v_, bi_ = f(gamma), f(beta), f(mean), f(var), f(bias_in)
            check(L.oadg_prep_conv_weights(ptr(w), ptr(g_), ptr(b_), ptr(m_), ptr(v_), float(eps), ptr(bi_), K, C, R, S,
                                           ptr(wf), ptr(wt), ptr(bias), ptr(scale), krsc, want_wt, stream_ptr()),
                  'oadg_prep_conv_weights')
            if entry is not None:
                entry.fill(w, g_, b_, m_, v_, float(eps), bi_, K, C, R, S, wf, wt, bias, scale, krsc, want_wt)
        ctx.save_for_backward(w, scale, m_, v_)
        # no zero tensors for the outputs nobody differentiates (autograd would otherwise fill a weight-sized zero
        # gradient for the transposed copy and a [K] one for an unused bias on every step); backward handles None
        ctx.set_materialize_grads(False)
        ctx.cfg = (float(eps), gamma is not None, bias_in is not None, K, C, R, S, krsc)
        ctx.leaf_inputs = leaf      # False: autograd ops (not AccumulateGrad) consume the gradients next
        ctx.wtoken = wtoken
        ctx.entry = entry
        if entry is not None:       # forward uses of these parameters in the current step (see DEFER_COLSUM)
            if entry.step != _STEP:
                entry.step, entry.count = _STEP, 0
            entry.count += 1
        if entry is not None:       # the bank's tensors live across steps: hand out fresh aliases (autograd stamps outputs)
            wf, bias, wt = wf.detach(), (bias.detach() if bias is not None else None), (wt.detach() if wt is not None else None)
        outs = (wf, bias if bias is not None else w.new_zeros(0), wt if wt is not None else w.new_zeros(0))
        ctx.mark_non_differentiable(outs[2])
        return outs

    @staticmethod
    def backward(ctx, gwf, gbias, _gwt):
        w, scale, mean, var = ctx.saved_tensors
        eps, has_bn, has_bias_in, K, C, R, S, krsc = ctx.cfg
        L = _lib.lib()
        dw = dgamma = dbeta = dbias_in = None
        gb = gbias.float().contiguous() if (gbias is not None and gbias.numel()) else None
        pend = pending_colsum(gbias)
        ent = ctx.entry
        if pend is not None and not (gb is gbias and _sole_use(ent, ctx.leaf_inputs)):
            resolve_colsum(gbias)       # the vector cannot wait (_sole_use)
            pend = None
        gb_now = None if pend is not None else gb
        flags = int(krsc) | (2 if pend is not None else 0)      # 2: dgamma is left raw for flush_colsums() to finish
        tok = ctx.wtoken
        parts = None
        if tok is not None and tok.parts is not None:
            parts, tok.parts = tok.parts, None
        if gwf is not None and isinstance(parts, _WgradJob) and ent is not None and ent.count > 1 and SHARED_GROUP and \
                DEFER_WGRAD and ctx.leaf_inputs and not has_bn and ent.step == _STEP and ent.expect_step == _STEP and \
                ent.expect_jobs > 1 and len(ent.shared) < ent.expect_jobs:
            # Round 5: a weight SHARED by several convolutions of the step (the RPN convolution: one weight, five pyramid
            # levels).  Its uses were launched one by one - autograd has to add their gradients - as single-job groups of a
            # few K-tiles per workgroup (4 launches, 0.49 ms at 845 TFLOP/s, + 4 consumer launches + 4 accumulation adds).
            # Now the uses' jobs wait on the bank entry; the LAST one puts them into the queue side by side: they run inside
            # one grouped launch, their split partials lie back to back in the group's workspace - the same [K][R*S][C] tiles
            # at the same stride - so ONE consumer job sums them as the splits of a single layer and returns the weight's
            # whole small-map gradient; the earlier uses return no gradient at all.  (The P2 use is a launch of its own,
            # its gradient is added by autograd as before.)
            ent.shared.append(parts)
            if len(ent.shared) < ent.expect_jobs:
                _SHARED_OPEN.add(ent)                # a member: launched and consumed with the group's last job
            else:
                dw = torch.empty_like(w)
                _enqueue_shared(ent, _Consumer(gbias=None, w=w, scale=scale, mean=mean, var=var, eps=eps, flags=flags,
                                               dw=dw.detach(), dgamma=None))
                flush_wgrads()       # now: autograd ADDS this gradient to the other uses' (it is read right away)
        elif gwf is not None and isinstance(parts, _WgradJob):
            # a small layer inside TrainEngine's backward: its weight gradient joins the current group
            defer = _sole_use(ent, ctx.leaf_inputs) and DEFER_WGRAD
            dw, dgamma = _attach_consumer(parts, ctx, gb_now, w, scale, mean, var, eps, flags, has_bn, record_targets=defer)
            _enqueue(parts)
            if not defer or _WQ_WORK >= WGRAD_GROUP:
                flush_wgrads()       # (not deferrable after all: the gradient is summed on arrival - run the group now)
        elif gwf is not None and parts is not None and DEFER_WGRAD and C * R * S <= MULTI_CONSUMER_LDS_FLOATS and \
                _sole_use(ent, ctx.leaf_inputs):
            # partials of a single-layer launch inside TrainEngine's backward: their consumer joins the group's (one launch
            # for all of them instead of one per layer - 14 launches of 9 - 22 us per step); it waits for that group's flush
            job = _WgradJob(C, K, R, S, parts=parts[0], splits=parts[1])
            dw, dgamma = _attach_consumer(job, ctx, gb_now, w, scale, mean, var, eps, flags, has_bn, record_targets=True)
            _enqueue(job)
        elif gwf is not None and parts is not None:        # fp32 split partials straight from the wgrad kernel
            dw, dgamma = _wgrad_dest(ctx, w, K, has_bn)      # w's strides (channels_last parameters keep theirs)
            check(L.oadg_prep_conv_weights_bwd_parts(ptr(parts[0]), parts[1], ptr(gb_now), ptr(w), ptr(scale), ptr(mean),
                                                     ptr(var), eps, K, C, R, S, ptr(dw), ptr(dgamma), flags, stream_ptr()),
                  'oadg_prep_conv_weights_bwd_parts')
        elif gwf is not None:
            gwf = gwf.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            dw, dgamma = _wgrad_dest(ctx, w, K, has_bn)
            check(L.oadg_prep_conv_weights_bwd(ptr(gwf), ptr(gb_now), ptr(w), ptr(scale), ptr(mean), ptr(var), eps, K, C,
                                               R, S, ptr(dw), ptr(dgamma), flags, stream_ptr()),
                  'oadg_prep_conv_weights_bwd')
        if pend is not None:
            src = ent.src
            pend.targets.append((src[2] if has_bn else src[-1], pend.out))
            if dgamma is not None:
                pend.fix = (dgamma.detach(), mean, var, float(eps))   # flush_colsums() finishes it from the raw dot product
                pend.targets.append((src[1], pend.fix[0]))
            # (dgamma None: the weight received no gradient; the vector itself is still the BN shift gradient)
        if has_bn:
            dbeta = gb
        elif has_bias_in:
            dbias_in = gb
        return dw, dgamma, dbeta, None, None, None, dbias_in, None, None, None


S2_DGRAD = os.environ.get('OADG_S2_DGRAD', '1') == '1'      # stride-2 data gradients on the csrc kernels (else MIOpen)


def _wt_useful(x, K, C, stride, pad, dil, R):
    """which second weight copy the data gradient of this convolution wants (``_PrepWeights`` ``want_wt``): 1 = flipped
    / transposed (stride 1), 2 = the four parity-class filters of a stride-2 3x3 / pad 1 or 1x1 / pad 0 layer, 0 = none
    (library data gradient)."""
    if not (x.requires_grad and K % 64 == 0 and C % 64 == 0):
        return 0
    if stride == 1 and dil * (R - 1) - pad >= 0:
        return 1
    if S2_DGRAD and stride == 2 and dil == 1 and ((R == 3 and pad == 1) or (R == 1 and pad == 0)):
        return 2
    return 0


class _BankEntry:
    """The prepared tensors of one trainable convolution, kept across steps (weights change only in optimizer.step()):
    ``valid`` while the version counters of the source parameters are the ones the tensors were prepared from."""
    __slots__ = ('src', 'versions', 'args', 'wf', 'wt', 'bias', 'scale', 'mean', 'var', 'want_wt', 'step', 'count',
                 'expect_jobs', 'expect_step', 'shared', '__weakref__')

    def __init__(self, src, want_wt):
        self.src, self.want_wt = src, int(want_wt)           # src: the tensors whose versions define validity
        self.versions = None
        self.step, self.count = -1, 0
        self.expect_jobs, self.expect_step, self.shared = 0, -1, []     # shared-weight weight-gradient group (below)
        self.wf = self.wt = self.bias = self.scale = self.mean = self.var = self.args = None

    def current_versions(self):
        return tuple((t._version, t.data_ptr()) for t in self.src)

    @property
    def valid(self):
        return self.versions is not None and self.versions == self.current_versions()

    def fill(self, w, g_, b_, m_, v_, eps, bi_, K, C, R, S, wf, wt, bias, scale, krsc, want_wt):
        # the bank re-reads the SOURCE tensors later: only layers whose kernel operands alias their parameters / buffers
        # (fp32, dense - no dtype or layout copy was made for the launch) can be refreshed in place
        ops = [w] + ([g_, b_, m_, v_] if g_ is not None else []) + ([bi_] if bi_ is not None else [])
        if len(ops) != len(self.src) or any(a.data_ptr() != s_.data_ptr() for a, s_ in zip(ops, self.src)):
            self.args = self.versions = None
            return
        self.args = (w, g_, b_, m_, v_, eps, bi_, K, C, R, S, krsc, want_wt)
        self.wf, self.wt, self.bias, self.scale, self.mean, self.var = wf, wt, bias, scale, m_, v_
        self.versions = self.current_versions()
        _BANK.register(self)


class _Bank:
    """All bank entries of the process + the device descriptor table of oadg_prep_conv_weights_multi."""

    def __init__(self):
        self.entries = weakref.WeakSet()
        self.table = None            # (device tensor, [entries in table order], total blocks)
        self.dirty = True

    def register(self, e):
        if e not in self.entries:
            self.entries.add(e)
        self.dirty = True            # (tensors of an entry may have been re-allocated)

    def refresh(self):
        """re-prepare every registered layer whose parameters changed, in ONE launch; returns the number of layers"""
        ents = []
        for e in self.entries:
            if e.args is None or not e.args[0].is_cuda:
                continue
            # the table holds RAW pointers of the source tensors: an entry whose parameter / buffer storage was re-pointed
            # since it was filled (p.data = ..., module.to(), load_state_dict(assign=True), parameter flattening) is
            # dropped here - never launched on the stale pointer, never re-stamped valid - and prepared again by its
            # next forward call
            if e.versions is None or any(v[1] != t.data_ptr() for v, t in zip(e.versions, e.src)):
                e.args = e.versions = None
                self.dirty = True
                continue
            ents.append(e)
        if not ents:
            self.table = None
            return 0
        if self.dirty or self.table is None or len(self.table[1]) != len(ents) or any(r() is None for r in self.table[1]):
            ents.sort(key=lambda e: e.wf.data_ptr())
            tab = np.zeros((len(ents),), _lib.PREP_DESC)
            p_ = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
            first = 0
            for i, e in enumerate(ents):
                w, g_, b_, m_, v_, eps, bi_, K, C, R, S, krsc, want_wt = e.args
                tab[i] = (p_(w), p_(g_), p_(b_), p_(m_), p_(v_), p_(bi_), p_(e.wf), p_(e.wt), p_(e.bias), p_(e.scale),
                          eps, K, C, R, S, krsc, want_wt, first)
                first += _lib.lib().oadg_prep_conv_weights_multi_blocks(K, C, R, S)
            dev = ents[0].wf.device
            t = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).to(dev)
            # (weak references: the table must not keep the layers of a model that was dropped alive)
            self.table, self.dirty = (t, [weakref.ref(e) for e in ents], first), False
        t, refs, total = self.table
        check(_lib.lib().oadg_prep_conv_weights_multi(ptr(t), len(refs), total, stream_ptr()),
              'oadg_prep_conv_weights_multi')
        for e in ents:
            e.versions = e.current_versions()
        return len(refs)


_BANK = _Bank()
PREP_BANK = True


def refresh_prepared():
    """Call right after optimizer.step(): one multi-layer launch re-prepares (BN fold, bf16 KRSC, data-gradient layouts)
    every trainable convolution, so that the next forward pass launches no weight preparation at all.  Layers whose
    parameters are changed by anything else afterwards (load_state_dict, manual edits - anything that bumps the tensors'
    version counters) are simply prepared again by their next forward call."""
    if not (ENABLED and PREP_BANK):
        return 0
    return _BANK.refresh()


def prepared(conv_weight, bn, bias_in, want_wt, cache_on=None):
    """(wf, bias, wt) for a convolution, BN-folded when ``bn`` is given.  Layers without trainable parameters are
    prepared once (``cache_on`` = the module that owns the weight); trainable ones keep their prepared tensors in a bank
    entry that ``refresh_prepared()`` updates after every optimizer step."""
    frozen = not (conv_weight.requires_grad or (bn is not None and (bn.weight.requires_grad or bn.bias.requires_grad))
                  or (bias_in is not None and bias_in.requires_grad))
    key = None
    if frozen and cache_on is not None:
        key = (conv_weight._version, conv_weight.data_ptr(), want_wt) + \
            ((bn.weight._version, bn.bias._version, bn.running_mean._version, bn.running_var._version)
             if bn is not None else ())
        c = getattr(cache_on, '_prepared', None)
        if c is not None and c[0] == key:
            return c[1]
    tok = None if frozen else WeightGradToken()
    entry = None
    if not frozen and cache_on is not None and PREP_BANK and conv_weight.dtype == torch.float32 and \
            all(t.grad_fn is None for t in (conv_weight, bias_in) if t is not None):
        entry = getattr(cache_on, '_oadg_prep_entry', None)
        if entry is None or entry.want_wt != int(want_wt) or entry.src[0] is not conv_weight:
            src = [conv_weight] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else []) + \
                ([bias_in] if bias_in is not None else [])
            entry = _BankEntry(src, want_wt)
            cache_on._oadg_prep_entry = entry
    if tok is not None:
        tok.deferrable = entry is not None
        tok.entry = entry
    if bn is not None:
        out = _PrepWeights.apply(conv_weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, None,
                                 want_wt, tok, entry)
    else:
        out = _PrepWeights.apply(conv_weight, None, None, None, None, 0.0, bias_in, want_wt, tok, entry)
    wf, bias, wt = out
    if tok is not None:
        wf._oadg_wtoken = tok
    out = (wf, bias if bias.numel() else None, wt if wt.numel() else None)
    if key is not None:
        cache_on._prepared = (key, out)
    return out


class GradToken:
    """Hand-off between the backward passes of two convolutions around one post-ReLU tensor t = relu(P(...)) whose
    ONLY consumers are a convolution C (and, optionally, the identity path of the block C opens):
    C's data-gradient kernel adds the identity-path gradient (``extra``, deposited by the block's last conv), applies
    the ReLU mask (t > 0) and reduces the bias gradient in its epilogue, so P neither masks nor reduces again.
    ``grad_ptr`` identifies the tensor C returned: if autograd delivers anything else to P (an unexpected extra
    consumer), P falls back to masking itself - masking twice is harmless, skipping it would not be.
    Several consumers (a stage output feeds the next stage's conv1, its downsample convolution and the FPN lateral):
    C = the conv1 is the FINISHER - its forward arms the token - and the other convolutions are DEPOSITORS
    (``dep_token``): a depositor whose backward runs while the token is armed and not yet closed computes its data
    gradient with the gradients deposited so far as the residual operand of its own epilogue, leaves the sum in
    ``extra`` and returns no gradient; the finisher adds ``extra`` in ITS epilogue (with the mask and the column sums) and
    closes the token.  Autograd's accumulation passes over the activation (13 per step, 0.8 ms) disappear.  Any other
    order stays correct: a depositor that finds the token closed (or never armed) returns its gradient as usual, autograd
    adds it, P then masks / reduces itself.  Every field but ``bits`` (P's forward) is written by these methods only."""
    __slots__ = ('extra', 'colsum', 'grad_ptr', 'bits', 'armed', 'closed', 'masked', 'adopted')

    def __init__(self, masked=True):
        self.extra = self.colsum = self.grad_ptr = self.bits = None
        self.armed = self.closed = self.adopted = False
        self.masked = masked        # False: t = P(...) without a ReLU (an FPN output): sums and column sums only

    def adopt(self):                    # P's forward (_Conv2dMFMA) received this token as its ``out_token``
        self.adopted = True

    def produced(self, t):
        """will a _Conv2dMFMA.backward claim this token for ``t``, the output of the call it went into as ``out_token``?"""
        return self.adopted and t.grad_fn is not None

    def arm(self):                      # the finisher's forward: its data gradient will finish the tensor's gradient
        self.armed = True

    def take(self):                     # a depositing convolution: the sum so far, for its own epilogue; then leave()
        extra, self.extra = self.extra, None
        return extra

    def leave(self, gx):
        self.extra = gx if gx.dtype == torch.bfloat16 else gx.to(torch.bfloat16)

    def close(self):                    # the finisher's backward, first thing, needed or not: what was left here
        self.closed = True
        return self.take()

    def finish(self, gx, colsum):       # ... after the launch that masked gx: P may trust exactly this tensor
        self.colsum, self.grad_ptr = colsum, gx.data_ptr()
        return gx

    def may_deposit(self):
        """a depositor asks first.  One running AFTER the finisher taints the token, whatever DEPOSIT says: autograd adds
        its returned gradient to the finisher's - possibly IN PLACE into the very tensor ``grad_ptr`` names (InputBuffer
        does when it holds the last reference), which P's pointer check could not see: P masks the sum itself."""
        if self.closed:
            self.grad_ptr = self.colsum = None
        return self.armed and not self.closed and DEPOSIT

    def deposit(self, g):
        """a gradient map computed elsewhere (RoIAlign): True = it stays here, False = the caller returns it"""
        ok = self.may_deposit() and g.dtype == torch.bfloat16
        if ok:
            self.extra = g if self.extra is None else self.extra + g
        return ok

    def hand_off(self, gy):             # the identity path of the block C opens (``res_token``): unconditional
        self.extra = gy

    def claim(self, gy):
        """P's backward -> (trusted, column sums): is ``gy`` the very tensor the finisher returned?  Clears the hand-off."""
        ok = self.grad_ptr is not None and self.grad_ptr == gy.data_ptr() and gy.dtype == torch.bfloat16 and \
            gy.is_contiguous(memory_format=torch.channels_last)
        colsum = self.colsum if ok else None
        self.grad_ptr = self.colsum = None
        return ok, colsum


RELU_BITS = True
DEPOSIT = True       # multi-consumer gradient sums inside the dgrad epilogues


def y_numel(x, w, stride, pad, dil):
    N, _, H, W = x.shape
    K, _, R, S = w.shape
    return N * K * ((H + 2 * pad - dil * (R - 1) - 1) // stride + 1) * ((W + 2 * pad - dil * (S - 1) - 1) // stride + 1)


def _incoming_grad(gy, y, out_token, wtoken, want_b):
    """step 1 of _Conv2dMFMA.backward -> (dy bf16 NHWC through the ReLU mask, bias gradient or None, bias gradient still
    wanted): claimed from the consumer's epilogue, or one pass of csrc/eltwise.hip, or torch where that does not apply"""
    trusted, colsum = out_token.claim(gy) if out_token is not None else (False, None)
    if trusted:
        gb = colsum if want_b else None               # masked and reduced by the consumer's dgrad epilogue
        if pending_colsum(gb) is not None and not (wtoken is not None and wtoken.uses == 1):
            resolve_colsum(gb)          # shared / unknown weights: autograd may sum this vector with others right away
        return gy, gb, False
    if (y is not None or want_b) and gy.dtype in (torch.bfloat16, torch.float32) and gy.shape[1] % 8 == 0 and \
            gy.is_contiguous(memory_format=torch.channels_last):
        return (*relu_bias_bwd(gy, y, want_b), False)               # mask + cast + bias gradient: one pass over dy
    gy = _nhwc_bf16(gy)
    if y is not None:
        gy = torch.ops.aten.threshold_backward(gy, y, 0)
    return gy, None, want_b


def _data_grad(gy, x16, wf, wt, stride, pad, dil, add, tok, deposit):
    """step 2 -> (dx, what torch still has to add to it).  ``add``: a gradient of the same tensor (deposited / handed over),
    summed in the launch's epilogue where the kernel takes one; ``tok``: the token to finish; ``deposit``: dx + add is
    complete on return (maybe in ``add``).  Without ``wt``: the library's dx for a depositor, else None (backward's call)."""
    R, kw = wf.shape[2], {}
    fin = wt is not None and tok is not None and (stride == 1 or (add is None and tok.masked))
    if fin:     # [* (x > 0): the producer's bits, else x itself], column sums -> the producer's bias gradient
        mb = tok.bits if tok.masked else None
        kw = dict(mask=x16 if (mb is None and tok.masked) else None, want_colsum=True, mask_bits=mb)
    if wt is None:
        if not deposit:
            return None, add
        gx = torch.ops.aten.convolution_backward(gy, x16, wf, None, [stride, stride], [pad, pad], [dil, dil], False,
                                                 [0, 0], 1, [True, False, False])[0]
    elif stride == 2 and deposit and R == 1 and add is not None:
        return conv_dgrad_s2(gy, wt, x16.shape, R, accumulate=add), None      # in place, on its strided grid
    elif stride == 2:   # Bottleneck.conv2 / downsample of a stage's first block: parity-class convolutions
        gx = conv_dgrad_s2(gy, wt, x16.shape, R, **kw)
    else:               # dx = conv(dy, rot180(W)^T) [+ add]
        gx, add = conv_forward(gy, wt, None, add, 1, dil * (R - 1) - pad, dil, False, **kw), None
    if fin:
        gx = tok.finish(*gx)
    if deposit and add is not None:
        gx, add = gx + add.to(gx.dtype), None
    return gx, add


def _weight_grad(wtok, x16, wf, gy, stride, pad, dil):
    """step 3 -> dW by the csrc kernels, in one of three forms (a job of the step's grouped launch, fp32 partials riding
    on the weight token, the finished gradient), or None: the library's"""
    K, C, R, S = wf.shape
    if not (x16.numel() < 2 ** 32 and _hip_wgrad(K, C)):
        return None
    if wtok is not None and wtok.uses == 1 and DEFER_WGRAD and \
            _group_sized(wtok.deferrable, x16, gy.shape[2], gy.shape[3], K, C, R, S):
        wtok.parts = _WgradJob(C, K, R, S, x16, gy, stride, pad, dil)  # launched with its group (flush_wgrads)
        return _dummy_grad(wf)
    if wtok is not None and wtok.uses == 1 and C * R * S * 4 <= PARTS_CONSUMER_LDS_BYTES:
        wtok.parts = conv_wgrad_parts(x16, gy, K, R, S, stride, pad, dil)
        return _dummy_grad(wf)          # the real gradient rides on the token (fp32 partials)
    return conv_wgrad(x16, gy, K, R, S, stride, pad, dil)


def _residual_grad(gy, rdt, res_token, res_up):
    """step 4: the residual operand's gradient is dy - handed to the block's first conv's data gradient (``res_token``),
    returned, or (``res_up``: the coarser FPN level's shape) summed 2 x 2"""
    gres = res_token.hand_off(gy) if res_token is not None else gy.to(rdt)       # (handed over: None)
    if res_up is not None:                    # d top[n, :, y, x] = sum of the 2 x 2 output gradients above it
        g16 = _nhwc_bf16(gy)
        gres = torch.empty(res_up, dtype=torch.bfloat16, device=gy.device, memory_format=torch.channels_last)
        check(_lib.lib().oadg_fpn_topdown_bwd(ptr(g16), ptr(gres), g16.shape[0], g16.shape[2], g16.shape[3], res_up[2],
                                              res_up[3], g16.shape[1], stream_ptr()), 'oadg_fpn_topdown_bwd')
        gres = gres.to(rdt)
    return gres


class _Conv2dMFMA(torch.autograd.Function):
    """y = [relu]( conv(x, wf) + bias [+ residual] ) in one kernel, on prepared bf16 weights.  Backward, the four steps
    above: ReLU mask + bias gradient in one pass (or taken over by the consumer through ``out_token``), data gradient on
    the csrc kernels with ``wt`` (+ the producer's mask / bias gradient / identity gradient through ``in_token``, or left
    on ``dep_token``), weight gradient by the csrc kernels; what is still needed then: ONE aten call (MIOpen)."""

    @staticmethod
    def forward(ctx, x, wf, bias, residual, wt, stride, pad, dil, relu, in_token, out_token, res_token, dep_token=None,
                res_up=False):
        x16 = _nhwc_bf16(x)
        if in_token is not None and wt is not None and stride == 1:
            in_token.arm()                  # this convolution's data gradient will finish the tensor's gradient
        if out_token is not None:
            out_token.adopt()
        r16 = _nhwc_bf16(residual) if residual is not None else None
        bits = None
        if relu and out_token is not None and RELU_BITS and wf.shape[0] % 8 == 0:
            # (y > 0) as one bit per element beside y: the consumer's data-gradient launch reads these instead of the
            # bf16 tensor for its ReLU-backward mask (1/16 of the bytes of an HBM-bound launch)
            bits = out_token.bits = torch.empty((y_numel(x16, wf, stride, pad, dil) // 8,), dtype=torch.uint8,
                                                device=x16.device)
        # res_up: ``residual`` is the coarser FPN level, added through the nearest 2x upsampling (fpn.py:166-175) in this
        # launch's epilogue; its gradient is the 2 x 2 sum of this convolution's output gradient (below)
        y = conv_forward(x16, wf, bias, r16, stride, pad, dil, relu, bits_out=bits, res_up=bool(res_up))
        ctx.res_up = tuple(r16.shape) if res_up else None
        ctx.save_for_backward(x16, wf, wt, y if relu else None)
        ctx.cfg = (stride, pad, dil, bias is not None, x.dtype, residual.dtype if residual is not None else None)
        ctx.tokens = (in_token, out_token, res_token, dep_token)
        ctx.wtoken = getattr(wf, '_oadg_wtoken', None)
        if ctx.wtoken is not None:
            ctx.wtoken.uses += 1
            ent = ctx.wtoken.entry
            if ent is not None and DEFER_WGRAD and SHARED_GROUP:
                # (a weight used by several convolutions of a step - the RPN convolution on every pyramid level: how many of
                #  its uses will hand a deferred job to _PrepWeights.backward)
                if ent.expect_step != _STEP:
                    ent.expect_step, ent.expect_jobs, ent.shared = _STEP, 0, []
                if _group_sized(ctx.wtoken.deferrable, x16, y.shape[2], y.shape[3], *wf.shape):
                    ent.expect_jobs += 1
        return y

    @staticmethod
    def backward(ctx, gy):
        x16, wf, wt, y = ctx.saved_tensors
        stride, pad, dil, has_bias, xdt, rdt = ctx.cfg
        in_token, out_token, res_token, dep_token = ctx.tokens
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gy, gb, want_b = _incoming_grad(gy, y, out_token, ctx.wtoken, has_bias and ctx.needs_input_grad[2])
        extra = in_token.close() if in_token is not None else None
        gx = gw = None
        if need_x and dep_token is not None and dep_token.may_deposit():
            # finished by another convolution: add what was deposited so far in THIS epilogue, leave the sum, return nothing
            dep_token.leave(_data_grad(gy, x16, wf, wt, stride, pad, dil, dep_token.take(), None, True)[0])
            need_x = False
        elif need_x:
            gx, extra = _data_grad(gy, x16, wf, wt, stride, pad, dil, extra, in_token, False)
            need_x = gx is None
        if need_w:
            gw = _weight_grad(ctx.wtoken, x16, wf, gy, stride, pad, dil)
            need_w = gw is None
            if want_b and not need_w:
                gb, want_b = gy.float().sum((0, 2, 3)), False
        if need_x or need_w or want_b:
            outs = torch.ops.aten.convolution_backward(
                gy, x16, wf, [wf.shape[0]] if has_bias else None, [stride, stride], [pad, pad], [dil, dil], False, [0, 0],
                1, [need_x, need_w, want_b])
            gx = outs[0] if gx is None else gx
            gw = outs[1] if outs[1] is not None else gw
            gb = outs[2].float() if outs[2] is not None else gb
        if gx is not None and extra is not None:      # library data gradient: the identity gradient is added here
            gx = gx + extra.to(gx.dtype)
        gres = _residual_grad(gy, rdt, res_token, ctx.res_up) if rdt is not None and ctx.needs_input_grad[3] else None
        return (gx.to(xdt) if gx is not None else None), gw, gb, gres, None, None, None, None, None, None, None, None, None, None


NARROW_HEAD = os.environ.get('OADG_NARROW_HEAD', '1') == '1'


def narrow_params(w_cat, b_cat):
    """(w16 bf16 [16, C], wt16 bf16 [C, 16], b16 fp32 [16]) of a 1x1 convolution with <= 16 output channels: the operands of
    csrc/narrow_head.hip (rows / entries past the live channels zero).  Built once per forward pass by the caller."""
    KN, C = w_cat.shape[0], w_cat.shape[1]
    with torch.no_grad():
        w16 = torch.zeros((16, C), dtype=torch.bfloat16, device=w_cat.device)
        w16[:KN].copy_(w_cat.detach().reshape(KN, C))
        wt16 = w16.t().contiguous()
        b16 = torch.zeros((16,), dtype=torch.float32, device=w_cat.device)
        if b_cat is not None:
            b16[:KN].copy_(b_cat.detach())
    return w16, wt16, b16


def _n16_launch(kind, M, C, extra_bytes, fn):
    """one launch of csrc/narrow_head.hip, with an event pair when bench.py times the kernel families"""
    e0 = _t0('n16')
    r = fn()
    if e0 is not None:
        # algorithmic bytes: the C-channel map and the 16-channel map once each (+ the mask bits of the data gradient)
        _t1(e0, 2.0 * M * C * 16, M * (2.0 * C + 32.0) + extra_bytes, 'n16_%s_kernel<%d>' % (kind, C),
            (1, M, 1, C, 16, 1, 1, False, kind == 'dgrad'))
    return r


class _NarrowHead(torch.autograd.Function):
    """ys[l] [N, 16, H_l, W_l] = conv1x1(xs[l], w) + b for a head with <= 16 output channels shared by the pyramid levels
    (the RPN head's rpn_cls + rpn_reg, rpn_head.py:54-68, anchor_head.py:147-163) on 16-channel-wide maps:
    csrc/narrow_head.hip forward / data gradient / weight gradient.  All levels are ONE autograd node: the weight / bias
    gradient partials of every level land in one buffer and are summed once (instead of a sum per level and autograd's
    accumulation of five gradients).  The data gradient of level l finishes ``toks[l]`` (ReLU mask bits + bias-gradient
    column sums of x_l = relu(rpn_conv(...))) like _Conv2dMFMA's does."""

    @staticmethod
    def forward(ctx, w_cat, b_cat, w16, wt16, b16, toks, *xs):
        L = _lib.lib()
        xs16, ys = [], []
        for x, tok in zip(xs, toks):
            x16 = _nhwc_bf16(x)
            N, C, H, W = x16.shape
            if tok is not None:
                tok.arm()
            y = torch.empty((N, 16, H, W), dtype=torch.bfloat16, device=x16.device, memory_format=torch.channels_last)
            check(_n16_launch('fwd', N * H * W, C, 0.0, lambda: L.oadg_conv1x1_n16_fwd(
                ptr(x16), ptr(w16), ptr(b16), ptr(y), N * H * W, C, stream_ptr())), 'oadg_conv1x1_n16_fwd')
            xs16.append(x16)
            ys.append(y)
        ctx.save_for_backward(wt16, *xs16)
        ctx.meta = (w_cat.shape[0], [x.dtype for x in xs], b_cat is not None)
        ctx.toks = list(toks)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        L = _lib.lib()
        wt16, *xs16 = ctx.saved_tensors
        KN, xdts, has_b = ctx.meta
        dev = wt16.device
        C = xs16[0].shape[1]
        gys = [_nhwc_bf16(g) if g is not None else torch.zeros((x.shape[0], 16) + tuple(x.shape[2:]), dtype=torch.bfloat16,
                                                              device=dev).contiguous(memory_format=torch.channels_last)
               for g, x in zip(gys, xs16)]
        Ms = [x.shape[0] * x.shape[2] * x.shape[3] for x in xs16]
        gxs = []
        for l, (x16, gy, tok, M) in enumerate(zip(xs16, gys, ctx.toks, Ms)):
            extra = tok.close() if tok is not None else None
            if not ctx.needs_input_grad[6 + l]:
                gxs.append(None)
                continue
            gx = torch.empty(x16.shape, dtype=torch.bfloat16, device=dev, memory_format=torch.channels_last)
            mb = tok.bits if (tok is not None and tok.masked) else None
            finish = tok is not None and extra is None and (mb is not None or not tok.masked)
            part = torch.empty((L.oadg_conv1x1_n16_dgrad_rows(M), C), dtype=torch.float32, device=dev) if finish else None
            check(_n16_launch('dgrad', M, C, M * C / 8.0 if (finish and mb is not None) else 0.0,
                              lambda: L.oadg_conv1x1_n16_dgrad(ptr(gy), ptr(wt16), ptr(gx), ptr(mb) if finish else None,
                                                               ptr(part), M, C, stream_ptr())), 'oadg_conv1x1_n16_dgrad')
            if finish:
                tok.finish(gx, _colsum(part, C))
            elif extra is not None:
                gx = gx + extra               # (another consumer deposited a gradient: the producer masks / reduces the sum)
            gxs.append(gx.to(xdts[l]))
        dw = db = None
        if ctx.needs_input_grad[0] or (has_b and ctx.needs_input_grad[1]):
            rows = [int(L.oadg_conv1x1_n16_wgrad_rows(M)) for M in Ms]
            part = torch.empty((sum(rows), 16, C), dtype=torch.float32, device=dev)
            bpart = torch.empty((sum(rows), 16), dtype=torch.float32, device=dev)
            z, off = _zeros(dev), 0
            for x16, gy, M, r in zip(xs16, gys, Ms, rows):
                check(_n16_launch('wgrad', M, C, 0.0, lambda: L.oadg_conv1x1_n16_wgrad(
                    ptr(x16), ptr(gy), ctypes.c_void_p(part.data_ptr() + off * 16 * C * 4),
                    ctypes.c_void_p(bpart.data_ptr() + off * 16 * 4), ptr(z), M, C, stream_ptr())), 'oadg_conv1x1_n16_wgrad')
                off += r
            dw = part.sum(0)[:KN].reshape(KN, C, 1, 1)
            if has_b:
                db = bpart.sum(0)[:KN]
        return (dw, db, None, None, None, None) + tuple(gxs)


def narrow_head_levels(xs, w_cat, b_cat, w16, wt16, b16, tokens=None):
    """the 16-channel head on every tensor of ``xs`` (one autograd node, see _NarrowHead): list of [N, 16, H, W] maps"""
    toks = list(tokens) if tokens is not None else [None] * len(xs)
    return list(_NarrowHead.apply(w_cat, b_cat, w16, wt16, b16, toks, *xs))


def narrow_head(x, w_cat, b_cat, w16, wt16, b16, in_token=None):
    return narrow_head_levels([x], w_cat, b_cat, w16, wt16, b16, [in_token])[0]


def _norm3(stride, padding, dilation):
    t = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)  # noqa: E731
    return t(stride), t(padding), t(dilation)


def _applies(x, weight, stride, padding, dilation):
    return supported(x, weight, stride, padding, dilation) and \
        (x.dtype == torch.bfloat16 or torch.is_autocast_enabled())     # fp32 parity runs keep fp32 arithmetic


def conv2d(x, weight, bias, stride, padding, dilation, relu=False, residual=None, owner=None, in_token=None,
           out_token=None, res_token=None, dep_token=None, res_up=False, bn=None):
    """layers.conv2d implementation hook: returns None for shapes the kernel does not cover.  ``bn``: see conv_bn"""
    stride, padding, dilation = _norm3(stride, padding, dilation)
    if not _applies(x, weight, stride, padding, dilation):
        return None
    K, C, R, S = weight.shape
    wf, b, wt = prepared(weight, bn, bias, _wt_useful(x, K, C, stride[0], padding[0], dilation[0], R), owner)
    return _Conv2dMFMA.apply(x, wf, b, residual, wt, stride[0], padding[0], dilation[0], bool(relu), in_token,
                             out_token, res_token, dep_token, bool(res_up))


def conv_bn(x, conv, bn, relu=False, residual=None, **tokens):
    """layers.conv_bn implementation hook (eval-mode BN folded by the preparation kernel)."""
    if bn.training or conv.bias is not None:
        return None
    return conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, relu, residual, conv, bn=bn, **tokens)


FUSED_FROZEN_BLOCK = os.environ.get('OADG_FUSED_FROZEN_BLOCK', '1') == '1'


def frozen_bottleneck(x, block):
    """A frozen bottleneck block of ResNet stage 1 as ONE launch (csrc/bottleneck_frozen.hip): the identity blocks
    (256 -> 64 -> 64 -> 256) and the stage's first block (64 -> 64 -> 64 -> 256 with the 1x1 downsample convolution on the
    shortcut), stride 1, eval-mode BN folded.  x is read once and y written once, where the three / four convolution
    launches move 2 - 4x the bytes (resnet.py:263-302 under _freeze_stages).  Returns None when the block / input is not
    of that kind - the caller runs its convolutions one by one.  No autograd graph: nothing upstream of a frozen block
    needs a gradient."""
    if not (on_path(x) and FUSED_FROZEN_BLOCK and x.dim() == 4 and not x.requires_grad):
        return None
    c1, c2, c3 = block.conv1, block.conv2, block.conv3
    ds = block.downsample
    cin = 256 if ds is None else 64
    if tuple(c1.weight.shape) != (64, cin, 1, 1) or tuple(c2.weight.shape) != (64, 64, 3, 3) or \
            tuple(c3.weight.shape) != (256, 64, 1, 1) or x.shape[1] != cin:
        return None
    convs, bns = [c1, c2, c3], [block.bn1, block.bn2, block.bn3]
    if ds is not None:
        if len(ds) != 2 or tuple(ds[0].weight.shape) != (256, 64, 1, 1):
            return None
        convs.append(ds[0])
        bns.append(ds[1])
    for c in convs:
        st, pd, dl = _norm3(c.stride, c.padding, c.dilation)
        if c.bias is not None or st != (1, 1) or dl != (1, 1) or pd != ((1, 1) if c is c2 else (0, 0)):
            return None
    if any(bn.training for bn in bns) or any(p.requires_grad for m in convs + bns for p in m.parameters()):
        return None
    # the fused launch bypasses the inner modules' forward(): a block whose convolutions / norms carry forward hooks
    # (feature taps, quantisation observers) runs them one by one.  OADG_FUSED_FROZEN_BLOCK=0: never fused.
    if any(m._forward_hooks or m._forward_pre_hooks for m in convs + bns + [block.relu]):
        return None
    folded = [prepared(c.weight, bn, None, 0, c) for c, bn in zip(convs, bns)]
    x16 = _nhwc_bf16(x)
    N, _, H, W = x16.shape
    y = torch.empty((N, 256, H, W), dtype=torch.bfloat16, device=x16.device, memory_format=torch.channels_last)
    (w1, b1, _), (w2, b2, _), (w3, b3, _) = folded[:3]
    L = _lib.lib()
    e0 = _t0('frozen_block')
    if ds is None:
        check(L.oadg_bottleneck_frozen_256(ptr(x16), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(y), N, H, W,
                                           stream_ptr()), 'oadg_bottleneck_frozen_256')
    else:
        wd, bd, _ = folded[3]
        check(L.oadg_bottleneck_frozen_first_64(ptr(x16), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(wd),
                                                ptr(bd), ptr(y), N, H, W, stream_ptr()), 'oadg_bottleneck_frozen_first_64')
    if e0 is not None:
        M = N * H * W
        # algorithmic work of the block: its convolutions without the halo recomputation; bytes: x read once, y written once
        _t1(e0, 2.0 * M * (cin * 64 + 64 * 64 * 9 + 64 * 256 + (64 * 256 if ds is not None else 0)), 2.0 * M * (cin + 256),
            'bottleneck_frozen_kernel' if ds is None else 'bottleneck_frozen_first_kernel',
            (N, H, W, cin, 256, 3, 1, ds is None, False))
    return y


ENABLED = False


def on_path(x):
    """is ``x`` on the bf16 MFMA path: kernels enabled, a device tensor, bf16 itself or under autocast?"""
    return ENABLED and x.is_cuda and (x.dtype == torch.bfloat16 or torch.is_autocast_enabled())


def tokens_ok(x, *convs):
    """may GradTokens be threaded through these convolutions of input x?  (all of them on the MFMA path, bf16/autocast,
    eval-mode BN folded, gradients flowing)"""
    if not (on_path(x) and torch.is_grad_enabled()):
        return False
    return all(c.bias is None and supported(x, c.weight, *_norm3(c.stride, c.padding, c.dilation)) for c in convs)


def enable(on=True):
    global ENABLED
    ENABLED = bool(on)
    from . import layers
    layers.set_conv_impl(conv2d if on else None, conv_bn if on else None)
