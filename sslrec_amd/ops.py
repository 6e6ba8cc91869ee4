"""torch.autograd bindings of the HIP kernels (libsslrec_hip.so through ctypes).

PyTorch is used for device memory, streams and autograd bookkeeping only; every
arithmetic step of the hot path runs in the hand-written gfx950 kernels.  There is NO
CPU or eager-PyTorch fallback: tensors must live on a HIP device and the shared object
must be built, otherwise these functions raise.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from .graph import BundledLayout, DroppedView, EdgePattern, PropGraph, RevaluedView, graph_of, pattern_of

# When set to a list, every SpMM launch appends (start_event, end_event, plan, d, has_acc): the
# measurement hook bench.py uses to time the dominant kernel with HIP events on the launch stream.
PROFILE = None
# An event record is a packet of its own on the launch stream (a few microseconds of bubble each): PROFILE_EVERY = n records a pair
# around every n-th SpMM launch only (n coprime with the launches of a step, so the sampled launch rotates through all of them); the
# other launches are still listed, with None for the two events
PROFILE_EVERY = 1
_profile_tick = 0


def _profile_this_launch():
    """False: the hook is off, or this launch is listed without events (PROFILE_EVERY); True: an event pair goes around it"""
    global _profile_tick
    if PROFILE is None:
        return False
    _profile_tick += 1
    return PROFILE_EVERY <= 1 or _profile_tick % PROFILE_EVERY == 0


# The same hook for the fused InfoNCE: when set to a list, every forward / backward call of _InfoNceFn appends
# (start_event, end_event, 'fwd' | 'bwd', B, M, d, variant word incl. precision and SSLREC_INFONCE_FWD_W) -- bench.py's MFMA roofline
# of the steps InfoNCE dominates (SimGCL, SGL)
PROFILE_INFONCE = None

# In-kernel launch timing for steps that are REPLAYED from a captured hipGraph (HIP events cannot be recorded inside one):
# when set to a StampLog, every SpMM launch is handed a 4 x uint64 device record in which the kernel itself accumulates its
# duration by the device's wall clock (include/sslrec_hip.h: sslrec_debug_stamp_next_launch); the record's address is baked
# into the captured launch, so after K replays it holds the sum over K executions.
STAMPS = None


class StampLog:
    def __init__(self, device, capacity=512):
        self.buf = torch.zeros((capacity, 4), dtype=torch.int64, device=device)
        self.buf[:, 0] = -1                      # running minimum of the start clocks
        self.meta = []
        self.khz = int(_lib.load().sslrec_debug_wall_clock_khz())

    def attach_next(self, *meta):
        if len(self.meta) >= self.buf.shape[0]:
            raise RuntimeError('StampLog is full (%d launches)' % self.buf.shape[0])
        rc = _lib.load().sslrec_debug_stamp_next_launch(self.buf[len(self.meta)].data_ptr())
        _lib.check(rc, 'sslrec_debug_stamp_next_launch')
        self.meta.append(meta)

    def reset_counts(self):
        """forget the executions so far (warm-up replays): sums and counts back to zero"""
        torch.cuda.synchronize(self.buf.device)
        self.buf[:, 1:] = 0
        self.buf[:, 0] = -1
        torch.cuda.synchronize(self.buf.device)

    def read(self):
        """[(meta, average duration in ms, executions)] of every launch that ran at least once"""
        host = self.buf.cpu().numpy()
        out = []
        for i, meta in enumerate(self.meta):
            n = int(host[i, 3])
            if n > 0:
                out.append((meta, float(host[i, 1]) / n / self.khz, n))
        return out

SPMM_DIMS = (32, 64, 128, 256)
# sslrec_epilogue_t.scale_flags (include/sslrec_hip.h): the factorized normalization of a layer chain on the column-swept kernel
SCALE_PATTERN, SCALE_Y, SCALE_ACC = 1, 2, 4
# SSLREC_SPMM_FACTORIZED=0: every launch of a layer chain reads the value stream (the round-1..4 form; bit-compatible with them).
# Default: when the adjacency's values factorize as r[i] * c[j] (PropGraph.factorization: the reference's D^-1/2 A D^-1/2 does), the
# chain carries the scaled table and only its first launch per direction reads values -- equal to rounding, not bit for bit.
# Chains with EmbedPerturb (SimGCL) keep the valued form unless SSLREC_SPMM_FACTORIZED=2: sign(y) (aug_utils.py:130) is discontinuous at 0,
# the valued chain adds the reference's own fp32 products in the reference's order (bit-equal to torch.spmm on almost every row), the
# factorized one rounds every term differently -- at amazon-book size that flipped the sign of about one element in 5.5e7 (call b:
# 201 gradient elements off by 1e-9 in the whole-step test), i.e. one perturbed element 0.2 away from the reference's.
FACTORIZED = {'0': 0, '1': 1, '2': 2}.get(os.environ.get('SSLREC_SPMM_FACTORIZED', '1'), 1)


def _chain_scale(adj, d, layer_num, perturbed=False):
    """row factor r [N] when the layer chain  E_l = A E_{l-1} / g_{l-1} = G + A^T g_l  over `adj` can run factorized: a plain or
    edge-dropped (values kept) view of a PropGraph whose values are r[i] * r[j], column-swept layouts in both directions, L >= 2;
    `perturbed`: the chain carries the EmbedPerturb epilogue (factorized only at level 2)"""
    if not FACTORIZED or layer_num < 2 or (perturbed and FACTORIZED < 2):
        return None
    if isinstance(adj, DroppedView):
        if adj.scale != 1.0:
            return None
        graph = adj.graph
    elif isinstance(adj, PropGraph):
        graph = adj
    else:
        return None
    if graph.bwd is None:
        return None
    fact = graph.factorization()
    if fact is None or not fact[2]:
        return None
    if graph.fwd.swept(d) is None or graph.bwd.swept(d) is None:
        return None
    return fact[0]
MAX_SUM_IN = 3          # SSLREC_MAX_SUM_IN: earlier layers' tables the last forward launch can add up (deferred layer sum)
# SSLREC_DEFERRED_SUM=1 (opt-in): the forward layer loop writes only E_l in the launches l < L and sums E0..E_L in the last one
# (swept layouts, 2 <= L <= 4; bit-identical to the running sum).  Measured in round 4 (EXPERIMENTS.md): 74 MB fewer bytes written per
# forward at amazon-book size, but the step is no faster (0.545-0.551 against 0.540-0.541 ms eager, 0.494-0.496 against 0.496-0.501 ms
# as one hipGraph) -- the last launch's flush waits for three table rows per output row instead of one -- so the running sum stays
# the default.
DEFERRED_SUM = os.environ.get('SSLREC_DEFERRED_SUM', '0') == '1'
# narrow tables (a GPU's d / P columns under feature slicing, sslrec_amd/feature_shard.py): column-swept kernel, and the
# row-bundled streamed kernel beyond that layout's size limits
SPMM_NARROW_DIMS = (8, 16)
INFONCE_DIMS = (32, 64, 128)
EVAL_KMAX = 64          # largest k of the fused evaluation kernel (csrc/eval.hip: per-user key buffers in LDS)
# arithmetic of the InfoNCE products, carried in bits 8..15 of the C ABI's `variant` (include/sslrec_hip.h);
# None = the process default (SSLREC_INFONCE_PRECISION, else h3 for the normalized variant 0 and x6 for LightGCL's variant 1)
INFONCE_PRECISIONS = {None: 0, 'x6': 1, 'fp32': 2, 'x36': 3, 'x3': 4, 'x63': 5, 'x6a': 6, 'h3': 7}
# SSLREC_INFONCE_FWD_W (bit 16 of `variant`): a forward that autograd will differentiate also accumulates the anchor-gradient sums
# W = sum_j exp(s_bj) all_j from the score tiles its row sums come from, and the backward does not recompute them (the B x M score
# products of a forward + backward: two instead of three).  A forward under no_grad / on tensors without requires_grad runs the
# plain row-sum kernel.  SSLREC_INFONCE_FWD_W=0 restores the three-pass form (A/B measurements).
INFONCE_FWD_W_BIT = 1 << 16
INFONCE_FWD_W = os.environ.get('SSLREC_INFONCE_FWD_W', '1') != '0'


def _variant_code(variant, precision):
    if precision not in INFONCE_PRECISIONS:
        raise ValueError('unknown InfoNCE precision %r (one of %s)' % (precision, sorted(k for k in INFONCE_PRECISIONS if k)))
    return int(variant) | (INFONCE_PRECISIONS[precision] << 8)


def _stream():
    return torch.cuda.current_stream().cuda_stream


_TICKET_WS = {}


def _ticket_ws(device, n_bytes, kind):
    """workspace of the one-launch reductions (sslrec_bpr_fwd_f32, sslrec_sumsq_fwd_f32): its first word is a ticket counter that must be 0
    at entry and that every call leaves 0 -- zeroed ONCE here and reused by every call of that kind on the device (a fresh torch.empty
    per call would need a fill launch per call; a hipGraph capture reuses the tensor its eager warm-up steps made, so no fill is
    captured either).  Calls on one stream are ordered; when the calling stream changes, the new stream first waits for the old one."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), kind)
    cur = torch.cuda.current_stream(dev)
    ent = _TICKET_WS.get(key)
    if ent is None or ent[0].numel() * 4 < n_bytes:
        ent = _TICKET_WS[key] = [torch.zeros(max(n_bytes // 4, 1), dtype=torch.float32, device=dev), cur]
    elif ent[1] != cur:
        if not torch.cuda.is_current_stream_capturing():      # (a capture starts behind a device-wide synchronize)
            cur.wait_stream(ent[1])
        ent[1] = cur
    return ent[0]


import collections
import threading

_KEPT_WS = collections.OrderedDict()      # (device, B, d) -> [workspace, stream]; least recently used first
_KEPT_WS_MAX = 8                          # (~1.7 MB + 12 B d bytes each -- variable batch sizes must not pile them up)
_KEPT_WS_LOCK = threading.Lock()          # (two Python threads must not initialise / evict at once; a workspace still serves one stream at a time)
SSLREC_KEPT_SCATTER = os.environ.get('SSLREC_KEPT_SCATTER', '1') != '0'      # 0: a fresh workspace + a clearing launch per BPR backward
# SSLREC_BPR_STAGED=0: the stacked BPR's forward computes the loss only and its backward stages and reduces (three launches, the form
# before); default: a forward that autograd will differentiate also stages the backward's rows (sslrec_bpr_fwd_staged_f32), two launches
BPR_STAGED = os.environ.get('SSLREC_BPR_STAGED', '1') != '0'
# SSLREC_REG_IN_FLUSH=0: propagate_sum's regularizer is always a launch of its own (sslrec_sumsq_fwd_f32); default: where the first
# forward product can carry it (sslrec_swept_sumsq_ok), its flush forms the sum from the E0 rows it reads anyway
REG_IN_FLUSH = os.environ.get('SSLREC_REG_IN_FLUSH', '1') != '0'
REG_ROUTES = {'flush': 0, 'kernel': 0}      # how often propagate_sum's regularizer took which route (tests, diagnostics)
# SSLREC_AXPY_BATCH=1 (opt-in): where the layout takes it (sslrec_swept_step_ok), a launch with an `axpy` operand requests its rows in
# batches beside the accumulator rows instead of one by one inside the flush (same bits).  Measured (EXPERIMENTS.md F.2): 0-1 us of
# the step eager, inside the spread of the other figures -- the launch pays for the 37 MB it reads, not for the round trips -- so the
# default stays the plain form.
AXPY_BATCH = os.environ.get('SSLREC_AXPY_BATCH', '0') == '1'
AXPY_ROUTES = {'batched': 0, 'plain': 0}


def _bpr_bwd_ws(device, B, d):
    """(workspace, kept): the BPR backward's staging rows + scatter table.  Kept per (device, B, d) and initialised once
    (sslrec_bpr_bwd_table_init): every call hands the table back clean, so a call is two launches instead of three.  Like the ticket
    workspaces it serves one stream at a time (a change of stream waits for the old one); batches beyond the table's 16,384
    contributions, or d > 256, take a fresh workspace and the ABI's own fallback."""
    lib = _lib.load()
    n = lib.sslrec_bpr_bwd_ws_bytes(B, d) // 4 + 1
    if not SSLREC_KEPT_SCATTER or 3 * B > 16384 or d > 256 or B <= 0:
        return torch.empty(n, dtype=torch.float32, device=device), False
    ws = _kept_ws(device, B, d)
    st = ws._sslrec_stage
    if st[1]:      # a forward staged its rows here and its backward has not run (and now cannot use them: the generation moves on)
        _lib.check(lib.sslrec_bpr_bwd_table_init(ws.data_ptr(), int(B), int(d), _stream()), 'sslrec_bpr_bwd_table_init')
        st[0], st[1] = st[0] + 1, False
    return ws, True


def _kept_ws(device, B, d):
    """the kept workspace itself.  It carries `_sslrec_stage` = [generation, staged]: `staged` = its scatter table holds the keys of a
    sslrec_bpr_fwd_staged_f32 that no backward has consumed yet, `generation` counts the stagings and their cancellations"""
    lib = _lib.load()
    n = lib.sslrec_bpr_bwd_ws_bytes(B, d) // 4 + 1
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(B), int(d))
    cur = torch.cuda.current_stream(dev)
    with _KEPT_WS_LOCK:
        ent = _KEPT_WS.get(key)
        if ent is None:
            ws = torch.empty(n, dtype=torch.float32, device=dev)
            _lib.check(lib.sslrec_bpr_bwd_table_init(ws.data_ptr(), int(B), int(d), _stream()), 'sslrec_bpr_bwd_table_init')
            ws._sslrec_stage = [0, False]
            ent = _KEPT_WS[key] = [ws, cur]
            while len(_KEPT_WS) > _KEPT_WS_MAX and not torch.cuda.is_current_stream_capturing():
                #  the dropped workspace was allocated on one stream and may last have been used on another (ent[1]): tell the
                # caching allocator, or it could hand the block back to the allocating stream while a backward on the other still reads it
                _k, old_ent = _KEPT_WS.popitem(last=False)
                if old_ent[1] is not None:
                    old_ent[0].record_stream(old_ent[1])
        else:
            _KEPT_WS.move_to_end(key)
            if ent[1] != cur:
                if not torch.cuda.is_current_stream_capturing():
                    cur.wait_stream(ent[1])
                ent[1] = cur
    return ent[0]


def _check_kept(rc, what, device, B, d):
    """like _lib.check; a kept-workspace call that failed may have left its scatter table dirty: forget the workspace, the next call
    initialises a fresh one"""
    if rc != 0:
        dev = torch.device(device)
        with _KEPT_WS_LOCK:
            _KEPT_WS.pop((dev.index if dev.index is not None else torch.cuda.current_device(), int(B), int(d)), None)
    _lib.check(rc, what)


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('sslrec_amd kernels run on a HIP device only (got a %s tensor); there is no CPU '
                               'fallback by design' % t.device)


def _f32c(t):
    if t.dtype != torch.float32:
        raise TypeError('fp32 tensors expected, got %s' % t.dtype)
    return t if t.is_contiguous() else t.contiguous()


def _idx(t):
    if t is None:
        return None
    if t.dtype != torch.int64:
        t = t.long()
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


# ----------------------------------------------------------------------------------------------
# raw launcher
# ----------------------------------------------------------------------------------------------
def spmm_raw(adj, x, which='fwd', y=None, noise=None, eps=0.0, acc_in=None, acc_out=None, want_y=True, chained=False,
             noise_sumsq=None, noise_geom=None, axpy=None, x_row_bits=None, sum_in=None, row_scale=None, scale_flags=0, reg_sumsq=None):
    """Launch one CSR SpMM with optional fused epilogue.  `adj` is a PropGraph or DroppedView;
    `which` selects A ('fwd') or A^T ('bwd').  Returns y (or None when want_y=False).  (`chained` is accepted and ignored.)
    Column slices of a table (feature-sliced tables): `noise_sumsq` [n_rows] = squared norm of the FULL noise row, `noise_geom`
    = (columns of the full table, first column of this slice) for the element index of computed (Philox) draws.
    `axpy` = (x [n_rows, d], alpha, scale tensor or None): acc_out += alpha * scale * x, fused (the regularizer's gradient).
    `x_row_bits` = RowBits or None: a hint that the rows of x outside the bitmap are all zeros (sslrec_epilogue_t.x_row_bits).
    `sum_in` = up to 3 tables: acc_out = ((acc_in + sum_in[0]) + ...) + y (deferred layer sum; column-swept layouts only).
    `row_scale` [n_rows] + `scale_flags` (SCALE_PATTERN | SCALE_Y | SCALE_ACC): the factorized normalization of a layer chain
    (sslrec_epilogue_t.scale_flags; column-swept layouts only).
    `reg_sumsq` = (ticket workspace, out [1], weight): the launch also writes out[0] = weight * sum(acc_in^2)
    (sslrec_spmm_swept_step_f32; the caller has asked sslrec_swept_step_ok)."""
    view = adj if isinstance(adj, (DroppedView, RevaluedView)) else None
    graph = adj.graph if view is not None else adj
    plan = getattr(graph, which)
    _need_gpu(x)
    x = _f32c(x)
    n, d = x.shape
    if n != plan.n_cols:
        raise ValueError('operand has %d rows, matrix has %d columns' % (n, plan.n_cols))
    if d not in SPMM_DIMS and d not in SPMM_NARROW_DIMS:
        raise ValueError('embedding size %d not supported by the raw HIP SpMM launcher (supported: %s and %s); the ops.spmm / '
                         'ops.propagate_sum wrappers zero-pad other sizes' % (d, SPMM_NARROW_DIMS, SPMM_DIMS))
    if want_y and y is None:
        y = torch.empty((plan.n_rows, d), dtype=torch.float32, device=x.device)
    epi = None
    keep_alive = []
    if noise is not None or acc_out is not None or x_row_bits is not None or scale_flags:
        epi = _lib.EpilogueStruct()
        if scale_flags:
            if row_scale is None or row_scale.numel() != plan.n_rows or row_scale.dtype != torch.float32 or not row_scale.is_contiguous():
                raise ValueError('row_scale: contiguous fp32 [%d] expected' % plan.n_rows)
            epi.row_scale, epi.scale_flags = row_scale.data_ptr(), int(scale_flags)
        if x_row_bits is not None:
            if x_row_bits.n_rows != n:
                raise ValueError('row bitmap of %d rows for an operand of %d rows' % (x_row_bits.n_rows, n))
            epi.x_row_bits = x_row_bits.bits.data_ptr()
        if noise_sumsq is not None:
            keep_alive.append(_f32c(noise_sumsq))
            epi.noise_sumsq = keep_alive[-1].data_ptr()
        if noise_geom is not None:
            epi.noise_row_stride, epi.noise_col_off = int(noise_geom[0]), int(noise_geom[1])
        if axpy is not None:
            ax, alpha, scale = axpy
            keep_alive.append(_f32c(ax))
            if tuple(keep_alive[-1].shape) != (plan.n_rows, d) or acc_out is None:
                raise ValueError('axpy operand of shape %s for an accumulator of shape %s' % (tuple(ax.shape), (plan.n_rows, d)))
            epi.axpy_x, epi.axpy_alpha = keep_alive[-1].data_ptr(), float(alpha)
            if scale is not None:
                keep_alive.append(scale.reshape(1).to(torch.float32).contiguous())
                epi.axpy_scale = keep_alive[-1].data_ptr()
        if noise is not None and not torch.is_tensor(noise):      # rng.PhiloxNoise: computed in the epilogue
            want = (plan.n_rows, d) if noise_geom is None else (plan.n_rows, int(noise_geom[0]))
            if tuple(noise.shape) != want:
                raise ValueError('noise of shape %s for an output of shape %s' % (noise.shape, want))
            epi.noise, epi.philox, epi.philox_stream = None, noise.state.state.data_ptr(), int(noise.stream)
        else:
            epi.noise = _ptr(_f32c(noise)) if noise is not None else None
        epi.eps = float(eps)
        epi.acc_in = _ptr(acc_in)
        epi.acc_out = _ptr(acc_out)
        if sum_in:
            if len(sum_in) > MAX_SUM_IN or acc_out is None:
                raise ValueError('at most %d deferred layer tables, and an accumulator to add them to' % MAX_SUM_IN)
            epi.n_sum_in = len(sum_in)
            for j, t in enumerate(sum_in):
                if tuple(t.shape) != (plan.n_rows, d) or not t.is_contiguous() or t.dtype != torch.float32:
                    raise ValueError('deferred layer table %d: contiguous fp32 [%d, %d] expected' % (j, plan.n_rows, d))
                epi.sum_in[j] = t.data_ptr()
    lib = _lib.load()
    swept = plan.swept(d)
    lay = col = val = r_len = w_len = None
    if swept is not None:
        if view is not None:
            col, val, w_len = view.masked(which, d)   # (pack, val, w_steps) overrides
    elif scale_flags:
        raise ValueError('the factorized normalization (scale_flags) is the column-swept kernel\'s')
    else:
        lay = plan.packed(d)
        if view is not None:
            col, val, r_len, w_len = view.compact(which, d)
    prof, ev0, ev1 = _profile_this_launch(), None, None
    if prof:                     # (an event pair of its own per launch: sharing one event between back-to-back launches would
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)      # charge the HOST's enqueue gaps of a
        ev0.record()                                                                               # launch-bound step to the kernel)
    if STAMPS is not None:
        STAMPS.attach_next(swept if swept is not None else lay, d, acc_out is not None, want_y, _entry_frac(view), None, len(sum_in or ()))
    if reg_sumsq is not None and (swept is None or epi is None):
        raise ValueError('reg_sumsq rides on a column-swept launch with an accumulator')
    step = None
    if reg_sumsq is not None:
        step = _lib.SweptStepStruct(reg_sumsq[0].data_ptr(), reg_sumsq[1].data_ptr(), float(reg_sumsq[2]), _lib.STEP_SUMSQ)
    elif (AXPY_BATCH and axpy is not None and swept is not None and swept.n_pass == 1 and not sum_in
          and lib.sslrec_swept_step_ok(C.byref(swept.c_struct()))):
        step = _lib.SweptStepStruct(None, None, 0.0, _lib.STEP_AXPY_BATCH)
        AXPY_ROUTES['batched'] += 1
    if axpy is not None and step is None:
        AXPY_ROUTES['plain'] += 1
    if swept is not None and step is not None:
        rc = lib.sslrec_spmm_swept_step_f32(C.byref(swept.c_struct()), _ptr(col), _ptr(val), _ptr(w_len), x.data_ptr(), d,
                                            _ptr(y) if want_y else None, C.byref(epi), C.byref(step), _stream())
        _lib.check(rc, 'sslrec_spmm_swept_step_f32')
    elif swept is not None:       # output table fits the chip's LDS: column-swept kernel (spmm_swept.hip)
        rc = lib.sslrec_spmm_swept_f32(C.byref(swept.c_struct()), _ptr(col), _ptr(val), _ptr(w_len), x.data_ptr(), d,
                                       _ptr(y) if want_y else None,
                                       C.byref(epi) if epi is not None else None, _stream())
        _lib.check(rc, 'sslrec_spmm_swept_f32')
    if swept is not None:
        if PROFILE is not None:
            if prof:
                ev1.record()
            PROFILE.append((ev0, ev1, swept, d, acc_out is not None, want_y, _entry_frac(view),
                            x_row_bits.max_rows if (x_row_bits is not None and epi is not None) else None, len(sum_in or ()),
                            bool(scale_flags & SCALE_PATTERN),
                            {'views': 1, 'perturbed': noise is not None, 'philox': noise is not None and not torch.is_tensor(noise), 'which': which}))
        return y if want_y else None
    if isinstance(lay, BundledLayout):      # narrow table beyond the swept layout: row-bundled kernel (spmm_bundle_kernel)
        # (col, val, b_steps, w_blocks) of a view: a compacted edge-dropped view brings all four, a re-valued one only the values
        rc = lib.sslrec_spmm_bundled_view_f32(C.byref(lay.c_struct()), _ptr(col), _ptr(val), _ptr(r_len), _ptr(w_len), x.data_ptr(), d,
                                              _ptr(y) if want_y else None, C.byref(epi) if epi is not None else None,
                                              _ptr(lay.partial_ws()), _stream())
        _lib.check(rc, 'sslrec_spmm_bundled_view_f32')
    else:
        rc = lib.sslrec_spmm_csr_f32(C.byref(lay.c_struct()), _ptr(col), _ptr(val), _ptr(r_len), _ptr(w_len),
                                     x.data_ptr(), d,
                                     _ptr(y) if want_y else None, C.byref(epi) if epi is not None else None,
                                     _ptr(lay.partial_ws()), _stream())
        _lib.check(rc, 'sslrec_spmm_csr_f32')
    if PROFILE is not None:
        if prof:
            ev1.record()
        PROFILE.append((ev0, ev1, lay, d, acc_out is not None, want_y, _entry_frac(view)))
    return y if want_y else None


def _entry_frac(view):
    """share of the matrix entries a launch reads (for the algorithmic-byte accounting of the measurement hook): 1 for
    the plain graph, the keep rate of a Philox edge-dropped view (its mask is never materialized)"""
    if isinstance(view, DroppedView) and view.keep is None:
        return float(view.philox[2])
    return 1.0


def _as_adj(adj):
    if isinstance(adj, (PropGraph, DroppedView, RevaluedView)):
        return adj
    return graph_of(adj)


# ----------------------------------------------------------------------------------------------
# Y = A X   (drop-in for torch.spmm in `_propagate`, reference lightgcn.py:28-29)
# ----------------------------------------------------------------------------------------------
class _SpmmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj):
        ctx.adj = adj
        return spmm_raw(adj, x, 'fwd')

    @staticmethod
    def backward(ctx, gy):
        return spmm_raw(ctx.adj, gy.contiguous(), 'bwd'), None


def _spmm_dim(adj, d):
    """embedding size the SpMM runs at: d itself when a kernel exists for it, else the next supported size (zero-padded)"""
    if d in SPMM_NARROW_DIMS:
        return d
    return _padded_dim(d, SPMM_DIMS)


def _padded_dim(d, supported):
    for s in supported:
        if d <= s:
            return s
    raise ValueError('embedding size %d exceeds the largest supported size %d' % (d, supported[-1]))


def _pad_cols(x, dp):
    """zero-pad the embedding dimension to a kernel-supported size (differentiable); zero columns
    change neither products, norms nor dot products, the result is sliced back by the caller"""
    d = x.shape[-1]
    return x if d == dp else torch.nn.functional.pad(x, (0, dp - d))


def spmm(adj, x):
    d = x.shape[1]
    adj = _as_adj(adj)
    dp = _spmm_dim(adj, d)
    y = _SpmmFn.apply(_pad_cols(x, dp), adj)
    return y if dp == d else y[:, :d]


# ----------------------------------------------------------------------------------------------
# learned edge weights (AdaptiveMask, reference aug_utils.py:52-80 as dccf.py:82-90 calls it): SDDMM, the row normalization
# of entry values, and a SpMM that is differentiable in its VALUES.  Per-entry arrays are fp32 [nnz] in the caller's entry
# order (the numbering of EdgeDrop masks and RevaluedView.vals); nothing of size nnz x d is ever stored.  (csrc/sddmm.hip)
# ----------------------------------------------------------------------------------------------
EDGE_DIMS = (8, 16, 32, 64, 128, 256)


def _pattern_graph(adj, what, device=None):
    """the PropGraph whose sparsity pattern `adj` carries; an edge-dropped view is refused (its pattern is not the graph's)"""
    adj = _as_adj(adj)
    if isinstance(adj, DroppedView):
        raise ValueError('%s: an edge-dropped view is not supported (an edge-dropped adaptive graph is out of scope)' % what)
    graph = adj.graph if isinstance(adj, RevaluedView) else adj
    gd = graph.device
    if device is not None and (gd.type != device.type or (gd.index is not None and device.index is not None and gd.index != device.index)):
        raise ValueError('%s: the graph lives on %s, the tensors on %s' % (what, graph.device, device))
    return graph


def _plan_of(graph, which, what):
    plan = getattr(graph, which) if which in ('fwd', 'bwd') else None
    if plan is None:
        raise ValueError('%s: the graph has no %r plan' % (what, which))
    return plan


def _entry_vec(t, nnz, what):
    t = _f32c(t)
    if t.dim() != 1 or t.numel() != nnz:
        raise ValueError('%s: fp32 [%d] in entry order expected, got %s' % (what, nnz, tuple(t.shape)))
    return t


def sddmm(adj, a, b, which='fwd', row_factor=None, col_factor=None):
    """out[e] = <a[row(e)], b[col(e)]> * row_factor[row(e)] * col_factor[col(e)] for every entry e of the pattern of `adj` (a PropGraph or
    a RevaluedView of one; which='bwd': of its transpose, so a has n_cols rows), fp32 [nnz] in the caller's entry order.  a and b may be
    the same table.  Not differentiable on its own: spmm_valued and edge_cosine_weights carry the gradients."""
    _need_gpu(a, b, row_factor, col_factor)
    graph = _pattern_graph(adj, 'sddmm', a.device)
    plan = _plan_of(graph, which, 'sddmm')
    a, b = _f32c(a.detach()), _f32c(b.detach())
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != plan.n_rows or b.shape[0] != plan.n_cols or a.shape[1] != b.shape[1]:
        raise ValueError('sddmm: operands of shapes %s and %s for a %d x %d pattern' % (tuple(a.shape), tuple(b.shape), plan.n_rows, plan.n_cols))
    d = a.shape[1]
    if d not in EDGE_DIMS:
        raise ValueError('embedding size %d not supported by the HIP SDDMM (supported: %s)' % (d, EDGE_DIMS))
    ra = None if row_factor is None else _f32c(row_factor.detach())
    cb = None if col_factor is None else _f32c(col_factor.detach())
    if (ra is not None and ra.numel() != plan.n_rows) or (cb is not None and cb.numel() != plan.n_cols):
        raise ValueError('sddmm: row_factor [%d] and col_factor [%d] expected' % (plan.n_rows, plan.n_cols))
    csr = plan.device_csr()
    out = torch.empty(plan.nnz, dtype=torch.float32, device=a.device)
    rc = _lib.load().sslrec_sddmm_f32(csr['row_of_entry'].data_ptr(), csr['col'].data_ptr(), csr['perm'].data_ptr(), plan.n_rows, plan.n_cols,
                                      plan.nnz, a.data_ptr(), b.data_ptr(), d, _ptr(ra), _ptr(cb), out.data_ptr(), _stream())
    _lib.check(rc, 'sslrec_sddmm_f32')
    return out


def row_invnorm(x, normalized=False):
    """n [N] = 1 / max(||x[r]||, 1e-12) (F.normalize's factor); normalized=True: (n, n (.) x)"""
    _need_gpu(x)
    x = _f32c(x.detach())
    n = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    xn = torch.empty_like(x) if normalized else None
    _lib.check(_lib.load().sslrec_row_invnorm_f32(x.data_ptr(), x.shape[0], x.shape[1], n.data_ptr(), _ptr(xn), _stream()),
               'sslrec_row_invnorm_f32')
    return (n, xn) if normalized else n


def _long(csr):
    lr = csr['long_rows']
    return (lr.data_ptr() if lr.numel() else None), lr.numel()


def _cosine_finish(s, n, g, p_a, p_b):
    """dS = n (.) (g - (p_a + p_b) (.) n (.) s), written over g"""
    _lib.check(_lib.load().sslrec_cosine_finish_f32(s.data_ptr(), n.data_ptr(), g.data_ptr(), p_a.data_ptr(), _ptr(p_b), s.shape[0], s.shape[1],
                                                    g.data_ptr(), _stream()), 'sslrec_cosine_finish_f32')
    return g


class _EdgeCosineFn(torch.autograd.Function):
    """w = rownorm((cos(head[row], tail[col]) + 1) / 2); saves c, w, inv_s and the inverse norms -- [nnz] and [N] vectors only"""

    @staticmethod
    def forward(ctx, head, tail, graph):
        square = tail is None
        h = _f32c(head)
        t = h if square else _f32c(tail)
        n_h = row_invnorm(h)
        n_t = n_h if square else row_invnorm(t)
        c = sddmm(graph, h, t, 'fwd', n_h, n_t)
        fwd = graph.fwd
        csr = fwd.device_csr()
        w = torch.empty_like(c)
        inv_s = torch.empty(fwd.n_rows, dtype=torch.float32, device=c.device)
        lr, n_long = _long(csr)
        _lib.check(_lib.load().sslrec_edge_rownorm_fwd_f32(csr['rowptr'].data_ptr(), csr['perm'].data_ptr(), fwd.n_rows, lr, n_long,
                                                           c.data_ptr(), w.data_ptr(), inv_s.data_ptr(), _stream()),
                   'sslrec_edge_rownorm_fwd_f32')
        ctx.graph, ctx.square = graph, square
        ctx.save_for_backward(h, t, c, w, inv_s, n_h, n_t)
        return w

    @staticmethod
    def backward(ctx, dw):
        h, t, c, w, inv_s, n_h, n_t = ctx.saved_tensors
        graph, square = ctx.graph, ctx.square
        fwd, bwd = graph.fwd, graph.bwd
        dw = _entry_vec(dw, fwd.nnz, 'edge_cosine_weights backward')
        cf, cb = fwd.device_csr(), bwd.device_csr()
        dc = torch.empty_like(c)
        p_head = torch.empty(fwd.n_rows, dtype=torch.float32, device=c.device)
        p_tail = torch.empty(fwd.n_cols, dtype=torch.float32, device=c.device)
        lr, n_long = _long(cf)
        lr_t, n_long_t = _long(cb)
        rc = _lib.load().sslrec_edge_rownorm_bwd_f32(cf['rowptr'].data_ptr(), cf['perm'].data_ptr(), fwd.n_rows, lr, n_long,
                                                     cb['rowptr'].data_ptr(), cb['perm'].data_ptr(), fwd.n_cols, lr_t, n_long_t,
                                                     dw.data_ptr(), w.data_ptr(), inv_s.data_ptr(), c.data_ptr(), dc.data_ptr(),
                                                     p_head.data_ptr(), p_tail.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_edge_rownorm_bwd_f32')
        view = RevaluedView(graph, dc)                           # the two valued SpMMs run on the tuned kernels
        if square:                                               # both ends from one table: the two parts add into one dS
            _, s_hat = row_invnorm(h, normalized=True)
            g = spmm_raw(view, s_hat, 'fwd')
            spmm_raw(view, s_hat, 'bwd', acc_in=g, acc_out=g, want_y=False)
            return _cosine_finish(h, n_h, g, p_head, p_tail), None, None
        _, h_hat = row_invnorm(h, normalized=True)
        _, t_hat = row_invnorm(t, normalized=True)
        d_h = _cosine_finish(h, n_h, spmm_raw(view, t_hat, 'fwd'), p_head, None)
        d_t = _cosine_finish(t, n_t, spmm_raw(view, h_hat, 'bwd'), p_tail, None)
        return d_h, d_t, None


def edge_cosine_weights(adj, head_table, tail_table=None):
    """AdaptiveMask's values (aug_utils.py:73-79) from NODE tables: w[e] = alpha[e] / sum of alpha over the row of e, alpha =
    (cos(head_table[row(e)], tail_table[col(e)]) + 1) / 2, an empty row's inverse sum being 0.  tail_table=None: both ends from one table
    (the square adjacency of DCCF).  Differentiable in the tables; fp32 [nnz] in the caller's entry order."""
    _need_gpu(head_table, tail_table)
    graph = _pattern_graph(adj, 'edge_cosine_weights', head_table.device)
    if graph.bwd is None:
        raise ValueError('edge_cosine_weights: the graph needs its transposed plan')
    n_rows, n_cols = graph.shape
    tail_rows = n_rows if tail_table is None else tail_table.shape[0]
    if head_table.dim() != 2 or head_table.shape[0] != n_rows or tail_rows != n_cols or \
            (tail_table is not None and tuple(tail_table.shape[1:]) != tuple(head_table.shape[1:])):
        raise ValueError('edge_cosine_weights: tables of %s / %s rows for a %d x %d pattern' % (head_table.shape[0], tail_rows, n_rows, n_cols))
    d = head_table.shape[1]
    dp = _padded_dim(d, EDGE_DIMS)                               # zero columns change neither norms nor dot products
    return _EdgeCosineFn.apply(_pad_cols(head_table, dp), None if tail_table is None else _pad_cols(tail_table, dp), graph)


class _SpmmValuedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vals, x, graph):
        vals, x = _entry_vec(vals, graph.nnz, 'spmm_valued'), _f32c(x)
        ctx.graph = graph
        ctx.save_for_backward(vals, x)
        return spmm_raw(RevaluedView(graph, vals), x, 'fwd')

    @staticmethod
    def backward(ctx, gy):
        vals, x = ctx.saved_tensors
        gy = _f32c(gy)
        dx = spmm_raw(RevaluedView(ctx.graph, vals), gy, 'bwd') if ctx.needs_input_grad[1] else None
        dvals = sddmm(ctx.graph, gy, x, 'fwd') if ctx.needs_input_grad[0] else None
        return dvals, dx, None


def spmm_valued(adj, vals, x):
    """Y = A(vals) X for the PATTERN of `adj` with the entry values `vals` (fp32 [nnz], caller's entry order; torch_sparse.spmm with
    learned values, dccf.py:89-90).  Differentiable in both: dX = A(vals)^T dY on the tuned SpMM, dvals[e] = <dY[row(e)], X[col(e)]> by
    SDDMM.  Embedding sizes without a kernel are zero-padded like ops.spmm."""
    _need_gpu(vals, x)
    graph = _pattern_graph(adj, 'spmm_valued', x.device)
    if graph.bwd is None:
        raise ValueError('spmm_valued: the graph needs its transposed plan')
    d = x.shape[1]
    dp = _spmm_dim(graph, d)
    y = _SpmmValuedFn.apply(vals, _pad_cols(x, dp), graph)
    return y if dp == d else y[:, :d]


# ----------------------------------------------------------------------------------------------
# intent-aware aggregation (dccf.py:77-80): Y = softmax(X C) C^T per row range of the stacked table, nothing of size N x K
# stored forward or backward (csrc/intent.hip)
# ----------------------------------------------------------------------------------------------
INTENT_DIMS = (32, 64, 128)
INTENT_KMAX = 256


class _IntentFn(torch.autograd.Function):
    """saves X, the matrices and ONE float per row (log-sum-exp of the logits); the backward recomputes the probabilities"""

    @staticmethod
    def forward(ctx, x, n_split, c_u, c_i):
        x = _f32c(x)
        c_u = None if c_u is None else _f32c(c_u)
        c_i = None if c_i is None else _f32c(c_i)
        n, d = x.shape
        k = (c_u if c_u is not None else c_i).shape[1]
        y = torch.empty_like(x)
        lse = torch.empty(n, dtype=torch.float32, device=x.device)
        if n > 0:                                                # (an empty tensor has no address to hand over)
            rc = _lib.load().sslrec_intent_fwd_f32(x.data_ptr(), n, n_split, d, _ptr(c_u), _ptr(c_i), k, y.data_ptr(), lse.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_intent_fwd_f32')
        ctx.n_split, ctx.has = n_split, (c_u is not None, c_i is not None)
        ctx.save_for_backward(x, lse, *[c for c in (c_u, c_i) if c is not None])
        return y

    @staticmethod
    def backward(ctx, gy):
        x, lse, *cs = ctx.saved_tensors
        cs = list(cs)
        c_u = cs.pop(0) if ctx.has[0] else None
        c_i = cs.pop(0) if ctx.has[1] else None
        gy = _f32c(gy)
        n, d = x.shape
        k = (c_u if c_u is not None else c_i).shape[1]
        lib = _lib.load()
        dx = torch.empty_like(x)
        dc_u = None if c_u is None else torch.empty_like(c_u)
        dc_i = None if c_i is None else torch.empty_like(c_i)
        if n == 0:
            return dx, None, (None if dc_u is None else dc_u.zero_()), (None if dc_i is None else dc_i.zero_())
        ws = torch.empty(lib.sslrec_intent_ws_bytes(n, ctx.n_split, d, k) // 4 + 1, dtype=torch.float32, device=x.device)
        rc = lib.sslrec_intent_bwd_f32(x.data_ptr(), gy.data_ptr(), lse.data_ptr(), n, ctx.n_split, d, _ptr(c_u), _ptr(c_i), k, dx.data_ptr(),
                                       _ptr(dc_u), _ptr(dc_i), ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_intent_bwd_f32')
        return dx, None, dc_u, dc_i


def _intent_matrix(c, what):
    if c.dim() != 2 or not 1 <= c.shape[1] <= INTENT_KMAX:
        raise ValueError('%s: an intent matrix [d, K] with 1 <= K <= %d expected, got %s' % (what, INTENT_KMAX, tuple(c.shape)))
    return c


def intent_aggregate_stacked(table, n_user, user_intent, item_intent):
    """concat([softmax(U @ user_intent, 1) @ user_intent.T, softmax(I @ item_intent, 1) @ item_intent.T]) for table = [U; I], U its first
    n_user rows (dccf.py:77-80): both products in ONE launch, no split / concat copies, no [N, K] tensor forward or backward.
    Differentiable in the table and both matrices ([d, K], K <= 256).  Embedding sizes without a kernel are zero-padded: zero columns
    of the table and zero rows of the matrices add nothing to any logit, the padded output columns are dropped."""
    _need_gpu(table, user_intent, item_intent)
    _intent_matrix(user_intent, 'intent_aggregate_stacked')
    _intent_matrix(item_intent, 'intent_aggregate_stacked')
    n_user = int(n_user)
    if table.dim() != 2 or not 0 <= n_user <= table.shape[0] or user_intent.shape != item_intent.shape or user_intent.shape[0] != table.shape[1]:
        raise ValueError('intent_aggregate_stacked: table %s, n_user %d, matrices %s / %s' %
                         (tuple(table.shape), n_user, tuple(user_intent.shape), tuple(item_intent.shape)))
    d = table.shape[1]
    dp = _padded_dim(d, INTENT_DIMS)
    pad_rows = lambda c: c if dp == d else torch.nn.functional.pad(c, (0, 0, 0, dp - d))
    y = _IntentFn.apply(_pad_cols(table, dp), n_user, pad_rows(user_intent), pad_rows(item_intent))
    return y if dp == d else y[:, :d]


def intent_aggregate(x, intents):
    """softmax(x @ intents, dim=1) @ intents.T for one table [N, d] and one matrix [d, K]; differentiable in both"""
    _need_gpu(x, intents)
    _intent_matrix(intents, 'intent_aggregate')
    if x.dim() != 2 or intents.shape[0] != x.shape[1]:
        raise ValueError('intent_aggregate: table %s, matrix %s' % (tuple(x.shape), tuple(intents.shape)))
    d = x.shape[1]
    dp = _padded_dim(d, INTENT_DIMS)
    c = intents if dp == d else torch.nn.functional.pad(intents, (0, 0, 0, dp - d))
    y = _IntentFn.apply(_pad_cols(x, dp), x.shape[0], c, None)
    return y if dp == d else y[:, :d]


# ----------------------------------------------------------------------------------------------
# hypergraph layer of HCCF (hccf.py:43-44, 48-49, 105-107): A = dropout(E W * mult), H = act(A^T X), Y = act(A H) per row range of the
# stacked tables, nothing of size N x K stored forward or backward, the dropout mask computed in the kernels (csrc/hyper.hip)
# ----------------------------------------------------------------------------------------------
HYPER_DIMS = (32, 64, 128)
HYPER_KMAX = 256


def hyper_fused_ok(d, k):
    """whether csrc/hyper.hip has kernels for the (padded) embedding size d and K hyperedges: at d = 128 with K > 128 not even two
    of the [d, K] matrices W, H, dQ fit the 160 KB of LDS, and hyper_propagate_stacked runs the composed torch expression instead"""
    return not (d == 128 and k > 128)


def hyper_keep_mask(state, stream, n_rows, k, keep_rate):
    """bool [n_rows, k]: the dropout mask the hypergraph kernels compute for call `stream` at the state's current step --
    floor(u + keep_rate) of EdgeDrop's arithmetic with u = Philox uniform number row * 4 ceil(k / 4) + col of the call (rows of the
    STACKED table).  For tests and for the composed fallback; the kernels never store it."""
    from .rng import philox_uniforms
    n_rows, k = int(n_rows), int(k)
    kp = (k + 3) // 4 * 4
    u = philox_uniforms(state, stream, n_rows * kp).view(n_rows, kp)[:, :k]
    return (u + keep_rate).floor().type(torch.bool)


def _hyper_composed(x, e, n_user, w_u, w_i, mult, leaky, keep_rate, mask):
    """the reference's expression (hccf.py:43-49, 105-107) with the given keep mask"""
    act = torch.nn.functional.leaky_relu

    def side(xr, er, w, m):
        a = er @ w * mult
        if m is not None:
            a = a * m.to(a.dtype) / keep_rate
        return act(a @ act(a.T @ xr, leaky), leaky)
    m_u, m_i = (None, None) if mask is None else (mask[:n_user], mask[n_user:])
    return torch.concat([side(x[:n_user], e[:n_user], w_u, m_u), side(x[n_user:], e[n_user:], w_i, m_i)], dim=0)


class _HyperFn(torch.autograd.Function):
    """saves X, E, the two matrices, Y and the two H ([d, K] each, kept transposed); the backward recomputes A and the mask"""

    @staticmethod
    def forward(ctx, x, e, n_split, w_u, w_i, mult, leaky, keep_rate, state, stream):
        x, e, w_u, w_i = _f32c(x), _f32c(e), _f32c(w_u), _f32c(w_i)
        n, d = x.shape
        k = w_u.shape[1]
        y = torch.empty_like(x)
        h_u, h_i = torch.zeros_like(w_u), torch.zeros_like(w_i)
        if n > 0:                                                # (an empty tensor has no address to hand over)
            lib = _lib.load()
            ws = torch.empty(lib.sslrec_hyper_ws_bytes(n, n_split, d, k) // 4 + 1, dtype=torch.float32, device=x.device)
            rc = lib.sslrec_hyper_fwd_f32(x.data_ptr(), e.data_ptr(), n, n_split, d, w_u.data_ptr(), w_i.data_ptr(), k, mult, leaky, keep_rate,
                                          _ptr(state), stream, h_u.data_ptr(), h_i.data_ptr(), y.data_ptr(), ws.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_hyper_fwd_f32')
        ctx.args = (n_split, mult, leaky, keep_rate, stream)
        ctx.state = state
        ctx.save_for_backward(x, e, w_u, w_i, y, h_u, h_i)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, e, w_u, w_i, y, h_u, h_i = ctx.saved_tensors
        n_split, mult, leaky, keep_rate, stream = ctx.args
        gy = _f32c(gy)
        n, d = x.shape
        k = w_u.shape[1]
        dx, de = torch.empty_like(x), torch.empty_like(e)
        dw_u, dw_i = torch.empty_like(w_u), torch.empty_like(w_i)
        if n == 0:
            return dx, de, None, dw_u.zero_(), dw_i.zero_(), None, None, None, None, None
        lib = _lib.load()
        ws = torch.empty(lib.sslrec_hyper_ws_bytes(n, n_split, d, k) // 4 + 1, dtype=torch.float32, device=x.device)
        rc = lib.sslrec_hyper_bwd_f32(x.data_ptr(), e.data_ptr(), gy.data_ptr(), y.data_ptr(), n, n_split, d, w_u.data_ptr(), w_i.data_ptr(),
                                      h_u.data_ptr(), h_i.data_ptr(), k, mult, leaky, keep_rate, _ptr(ctx.state), stream, dx.data_ptr(),
                                      de.data_ptr(), dw_u.data_ptr(), dw_i.data_ptr(), ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_hyper_bwd_f32')
        return dx, de, None, dw_u, dw_i, None, None, None, None, None


def hyper_propagate_stacked(x, e, n_user, user_hyper, item_hyper, mult, leaky, keep_rate, rng=None):
    """One hypergraph layer of HCCF on the stacked tables x, e = [U; I] [N, d] (hccf.py:43-44, 48-49, 105-107): with
    A = dropout(e_r @ W_r * mult, p = 1 - keep_rate), W_r = user_hyper for the first n_user rows and item_hyper for the rest ([d, K]),
    returns concat over the two ranges of act(A @ act(A.T @ x_r)), act = LeakyReLU(leaky).  Differentiable in x, e and both matrices;
    no [N, K] tensor forward or backward.  rng = (rng.PhiloxState, stream): the dropout mask is computed in the kernels from that
    call's Philox stream (hyper_keep_mask writes the same mask out); required when keep_rate < 1.  The backward recomputes the mask from
    the LIVE state tensor, not from a snapshot: the state must not advance() between this call and its backward (a training step
    advances once, before its forward), or the gradients belong to another mask.  Embedding sizes without a kernel
    are zero-padded; a shape that does not fit LDS (hyper_fused_ok) runs the composed torch expression with the same mask."""
    _need_gpu(x, e, user_hyper, item_hyper)
    n_user, mult, leaky, keep_rate = int(n_user), float(mult), float(leaky), float(keep_rate)
    if not leaky > 0.0:
        raise ValueError('hyper_propagate_stacked: leaky must be positive (the backward reads the slope from the sign of the output), got %r' % leaky)
    if not 0.0 < keep_rate <= 1.0:
        raise ValueError('hyper_propagate_stacked: keep_rate must lie in (0, 1], got %r' % keep_rate)
    if x.dim() != 2 or e.shape != x.shape or not 0 <= n_user <= x.shape[0] or user_hyper.dim() != 2 or user_hyper.shape != item_hyper.shape \
            or user_hyper.shape[0] != x.shape[1] or not 1 <= user_hyper.shape[1] <= HYPER_KMAX:
        raise ValueError('hyper_propagate_stacked: tables %s / %s, n_user %d, matrices %s / %s ([d, K], 1 <= K <= %d)' %
                         (tuple(x.shape), tuple(e.shape), n_user, tuple(user_hyper.shape), tuple(item_hyper.shape), HYPER_KMAX))
    state, stream = None, 0
    if keep_rate < 1.0:
        if rng is None:
            raise ValueError('hyper_propagate_stacked: keep_rate < 1 needs rng = (PhiloxState, stream)')
        state, stream = rng[0].state, int(rng[1])
    d, k = x.shape[1], user_hyper.shape[1]
    dp = _padded_dim(d, HYPER_DIMS)
    if not hyper_fused_ok(dp, k):
        mask = None if state is None else hyper_keep_mask(rng[0], stream, x.shape[0], k, keep_rate)
        return _hyper_composed(x, e, n_user, user_hyper, item_hyper, mult, leaky, keep_rate, mask)
    pad_rows = lambda w: w if dp == d else torch.nn.functional.pad(w, (0, 0, 0, dp - d))
    y = _HyperFn.apply(_pad_cols(x, dp), _pad_cols(e, dp), n_user, pad_rows(user_hyper), pad_rows(item_hyper), mult, leaky, keep_rate, state,
                       stream)
    return y if dp == d else y[:, :d]


# ----------------------------------------------------------------------------------------------
# graph-transformer layer of AutoCF / GFormer (autocf.py:109-129) on projected NODE tables: an edge attention over a sparse pattern,
# nothing of size E x d or E x H stored forward or backward, no atomics (csrc/gt.hip)
# ----------------------------------------------------------------------------------------------
GT_DIMS = (32, 64, 128)
GT_HEAD_DIMS = (4, 8, 16, 32, 64, 128)


def edge_attention_fused_ok(d, head_num):
    """whether csrc/gt.hip has kernels for embedding size d with head_num heads; other shapes run the composed torch expression"""
    return d in GT_DIMS and d % head_num == 0 and d // head_num in GT_HEAD_DIMS


def _edge_attention_composed(pattern, q, k, v, head_num):
    """the reference's expression (autocf.py:119-128) on the node tables: [E, d] intermediates and index_add_"""
    n, d = q.shape
    rows, cols = pattern.coo()
    dh = d // head_num
    qe, ke, ve = (x.view(-1, head_num, dh) for x in (q[rows], k[cols], v[cols]))
    att = torch.exp(torch.clamp(torch.einsum('ehd, ehd -> eh', qe, ke), -10.0, 10.0))
    norm = torch.zeros(n, head_num, dtype=q.dtype, device=q.device).index_add_(0, rows, att)[rows]
    att = att / (norm + 1e-8)
    res = torch.einsum('eh, ehd -> ehd', att, ve).reshape(-1, d)
    return torch.zeros(n, d, dtype=q.dtype, device=q.device).index_add_(0, rows, res)


class _EdgeAttentionFn(torch.autograd.Function):
    """saves Q, K, V, Y and Z ([N, H]: the row sums of the exponentials); the backward recomputes every score"""

    @staticmethod
    def forward(ctx, q, k, v, pattern, head_num):
        q, k, v = _f32c(q), _f32c(k), _f32c(v)
        n, d = q.shape
        y = torch.empty_like(q)
        z = torch.empty(n, head_num, dtype=torch.float32, device=q.device)
        if n > 0:                                                # (an empty tensor has no address to hand over)
            p = pattern
            rc = _lib.load().sslrec_gt_fwd_f32(p.rowptr.data_ptr(), p.col.data_ptr(), n, _ptr(p.long_rows) if p.long_rows.numel() else None,
                                               p.long_rows.numel(), q.data_ptr(), k.data_ptr(), v.data_ptr(), d, head_num, y.data_ptr(),
                                               z.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_gt_fwd_f32')
        ctx.pattern, ctx.head_num = pattern, head_num
        ctx.save_for_backward(q, k, v, y, z)
        return y

    @staticmethod
    def backward(ctx, gy):
        q, k, v, y, z = ctx.saved_tensors
        p, head_num = ctx.pattern, ctx.head_num
        gy = _f32c(gy)
        n, d = q.shape
        dq, dk, dv = (torch.empty_like(q) if need else None for need in ctx.needs_input_grad[:3])
        if n > 0 and (dq is not None or dk is not None or dv is not None):
            t_ws = torch.empty(n * head_num, dtype=torch.float32, device=q.device)
            rc = _lib.load().sslrec_gt_bwd_f32(p.rowptr.data_ptr(), p.col.data_ptr(), _ptr(p.long_rows) if p.long_rows.numel() else None,
                                               p.long_rows.numel(), p.colptr.data_ptr(), p.row.data_ptr(),
                                               _ptr(p.long_cols) if p.long_cols.numel() else None, p.long_cols.numel(), n, q.data_ptr(),
                                               k.data_ptr(), v.data_ptr(), y.data_ptr(), z.data_ptr(), gy.data_ptr(), d, head_num, _ptr(dq) or None,
                                               _ptr(dk) or None, _ptr(dv) or None, t_ws.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_gt_bwd_f32')
        return dq, dk, dv, None, None


def edge_attention(pattern, q, k, v, head_num):
    """Y [N, d] of the graph-transformer layer (autocf.py:109-129, gformer.py:221-255) from the projected NODE tables q, k, v [N, d]
    (the reference projects the [E, d] gathers; (X[rows]) W = (X W)[rows]): per entry e = (r, c) of `pattern` and head h,
    a = exp(clamp(<q[r, h], k[c, h]>, -10, 10)) / (sum of the exponentials over row r + 1e-8), Y[r, h] = sum over the row of a * v[c, h];
    rows without entries are exact zeros.  `pattern`: a graph.EdgePattern (square, no duplicate entries) or a torch sparse adjacency
    (its pattern is built once and cached on the tensor).  Differentiable in q, k, v; nothing of size E x d or E x H is stored and two
    runs give the same bits.  d in {32, 64, 128} with d / head_num in {4, ..., 128} run csrc/gt.hip; any other shape runs the composed
    torch expression (edge_attention_fused_ok)."""
    _need_gpu(q, k, v)
    if not isinstance(pattern, EdgePattern):
        pattern = pattern_of(pattern)
    head_num = int(head_num)
    if q.dim() != 2 or q.shape != k.shape or q.shape != v.shape or q.shape[0] != pattern.n:
        raise ValueError('edge_attention: tables %s / %s / %s for a pattern of %d nodes' % (tuple(q.shape), tuple(k.shape), tuple(v.shape), pattern.n))
    d = q.shape[1]
    if head_num < 1 or d % head_num != 0:
        raise ValueError('edge_attention: the embedding size %d is not a multiple of head_num = %d' % (d, head_num))
    dev = q.device
    if pattern.device.type != dev.type or (pattern.device.index is not None and dev.index is not None and pattern.device.index != dev.index):
        raise ValueError('edge_attention: the pattern lives on %s, the tensors on %s' % (pattern.device, dev))
    q, k, v = (x.float().contiguous() for x in (q, k, v))
    if not edge_attention_fused_ok(d, head_num):
        return _edge_attention_composed(pattern, q, k, v, head_num)
    return _EdgeAttentionFn.apply(q, k, v, pattern, head_num)


# ----------------------------------------------------------------------------------------------
# AdaGCL's two view generators on [nnz] and [N] vectors: the VGAE edge decoder over all entries (adagcl.py:221-237, csrc/edgemlp.hip)
# and DenoiseNet's edge gate with its symmetric normalisation (adagcl.py:274-338, :358-401, :340-347, csrc/gate.hip).  Nothing of
# size nnz x d is stored; per-entry arrays are fp32 [nnz] in the caller's entry order.
# ----------------------------------------------------------------------------------------------
EDGE_MLP_DIMS = INTENT_DIMS
EDGE_MLP_FUSED = os.environ.get('SSLREC_EDGE_MLP_FUSED', '1') != '0'      # 0: the composed torch expression at every size (measurement)
EDGE_GATE_FUSED = os.environ.get('SSLREC_EDGE_GATE_FUSED', '1') != '0'


def edge_mlp_fused_ok(d):
    """whether csrc/edgemlp.hip has a decoder kernel for embedding size d; any other size runs the composed torch expression"""
    return EDGE_MLP_FUSED and d in EDGE_MLP_DIMS


def _edge_mlp_composed(csr, x, w1, b1, w2, b2):
    """the reference's expression (adagcl.py:166, :224) with its [nnz, d] intermediates, in the caller's entry order"""
    relu = torch.nn.functional.relu
    rows, cols = csr['row_of_entry'].long(), csr['col'].long()
    hidden = relu(torch.nn.functional.linear(relu(x[rows] * x[cols]), w1, b1))
    out = torch.empty(rows.shape[0], dtype=torch.float32, device=x.device)
    out[csr['perm'].long()] = hidden @ w2 + b2
    return out


def edge_mlp_logits(adj, x, w1, b1, w2, b2):
    """logit[e] = w2 . relu(W1 relu(x[row(e)] (.) x[col(e)]) + b1) + b2 for every entry e of the square pattern of `adj` (a PropGraph, a
    RevaluedView of one or a torch sparse adjacency): the VGAE decoder of AdaGCL before its sigmoid (adagcl.py:166, :224), fp32 [nnz] in
    the caller's entry order.  x [N, d], w1 [d, d] and b1 [d] as nn.Linear holds them, w2 [d] or [1, d], b2 a one-element tensor.  Not
    differentiable, like ops.sddmm (the reference calls it under no_grad).  d in {32, 64, 128} runs csrc/edgemlp.hip, which also leaves
    the keep flags logit >= 0 and their per-workgroup counts on the returned tensor for edge_keep_view; the reference's
    floor(sigmoid(logit) + 0.5) differs from that flag only for fp32 logits within a few 2^-23 below 0, where the fp32 sigmoid has
    already rounded to 0.5.  Any other d runs the composed torch expression (edge_mlp_fused_ok)."""
    _need_gpu(x, w1, b1, w2, b2)
    graph = _pattern_graph(adj, 'edge_mlp_logits', x.device)
    plan = graph.fwd
    x, w1, b1, w2, b2 = (_f32c(t.detach()) for t in (x, w1, b1, w2.reshape(-1), b2.reshape(-1)))
    d = x.shape[1] if x.dim() == 2 else -1
    if x.dim() != 2 or plan.n_rows != plan.n_cols or x.shape[0] != plan.n_rows or tuple(w1.shape) != (d, d) or b1.numel() != d or \
            w2.numel() != d or b2.numel() != 1:
        raise ValueError('edge_mlp_logits: x %s, W1 %s, b1 [%d], w2 [%d], b2 [%d] for a %d x %d pattern' %
                         (tuple(x.shape), tuple(w1.shape), b1.numel(), w2.numel(), b2.numel(), plan.n_rows, plan.n_cols))
    csr = plan.device_csr()
    if not edge_mlp_fused_ok(d):
        return _edge_mlp_composed(csr, x, w1, b1, w2, b2)
    logit = torch.empty(plan.nnz, dtype=torch.float32, device=x.device)
    keep = torch.empty(plan.nnz, dtype=torch.uint8, device=x.device)
    counts = torch.empty(_lib.EDGE_MLP_SLOTS, dtype=torch.int32, device=x.device)
    n_counts = C.c_int32(0)
    rc = _lib.load().sslrec_edge_mlp_fwd_f32(csr['row_of_entry'].data_ptr(), csr['col'].data_ptr(), csr['perm'].data_ptr(), plan.n_rows,
                                             plan.n_cols, plan.nnz, x.data_ptr(), d, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                             logit.data_ptr(), keep.data_ptr(), counts.data_ptr(), C.byref(n_counts), _stream())
    _lib.check(rc, 'sslrec_edge_mlp_fwd_f32')
    logit._sslrec_keep = (keep, counts, int(n_counts.value))
    return logit


def edge_keep_view(adj, logits):
    """(view, keep, kept) of vgae_generate (adagcl.py:229-237): keep [nnz] uint8 = logits >= 0, kept = their number (an int32 device
    tensor of one element: no host round trip) and `view`, a RevaluedView of the cached plan of `adj` with the values
    vals[e] * keep[e] / (kept / nnz) -- the dropped entries get the value 0, no new plan is built.  A view that keeps nothing has the
    value 0 everywhere (the reference divides by 0); whoever reads `kept` on the host decides what that means."""
    _need_gpu(logits)
    graph = _pattern_graph(adj, 'edge_keep_view', logits.device)
    nnz = graph.nnz
    stash = getattr(logits, '_sslrec_keep', None)
    logits_c = _entry_vec(logits.detach(), nnz, 'edge_keep_view')
    lib = _lib.load()
    if nnz == 0:
        raise ValueError('edge_keep_view: the pattern has no entries')
    if stash is not None and stash[0].numel() == nnz:
        keep, counts, n_counts = stash
    else:
        keep = torch.empty(nnz, dtype=torch.uint8, device=logits.device)
        counts = torch.empty(_lib.EDGE_MLP_SLOTS, dtype=torch.int32, device=logits.device)
        n = C.c_int32(0)
        _lib.check(lib.sslrec_edge_keep_flags(logits_c.data_ptr(), nnz, keep.data_ptr(), counts.data_ptr(), C.byref(n), _stream()),
                   'sslrec_edge_keep_flags')
        n_counts = int(n.value)
    vals = getattr(graph, '_entry_vals', None)
    if vals is None:                                             # the adjacency's own values in the caller's entry order, once per graph
        fwd = graph.fwd
        host = np.empty(nnz, dtype=np.float32)
        host[fwd.perm_host] = fwd.csr_val_host
        vals = graph._entry_vals = torch.from_numpy(host).to(graph.device)
    out = torch.empty(nnz, dtype=torch.float32, device=logits.device)
    kept = torch.empty(1, dtype=torch.int32, device=logits.device)
    _lib.check(lib.sslrec_edge_keep_finish_f32(vals.data_ptr(), keep.data_ptr(), counts.data_ptr(), n_counts, nnz, out.data_ptr(),
                                               kept.data_ptr(), _stream()), 'sslrec_edge_keep_finish_f32')
    return RevaluedView(graph, out), keep, kept


def _edge_gate_composed(csr, n, p, q, bias, gamma, zeta, beta, noise, eps):
    """the reference's expression (adagcl.py:294-311, :328-334, :340-347) on the entry list, in the caller's entry order"""
    rows, cols, perm = csr['row_of_entry'].long(), csr['col'].long(), csr['perm'].long()
    la = p[rows] + q[cols] + bias
    g = la if noise is None else (noise[perm] + la) / beta
    m = torch.clamp(torch.sigmoid(g) * (zeta - gamma) + gamma, 0.0, 1.0)
    s = torch.zeros(n, dtype=m.dtype, device=m.device).index_add(0, rows, m) + eps
    dinv = torch.clamp(torch.pow(s, -0.5), 0.0, 10.0)
    vals = torch.zeros_like(m).index_copy(0, perm, m * dinv[rows] * dinv[cols])
    l0 = torch.sigmoid(la - beta * math.log(-gamma / zeta)).mean()
    return vals, l0


class _EdgeGateFn(torch.autograd.Function):
    """saves p, q, bias, the noise, the gates m [nnz] and s, dinv [N]: [nnz] and [N] vectors only; the backward recomputes log_alpha"""

    @staticmethod
    def forward(ctx, p, q, bias, noise, graph, gamma, zeta, beta, eps):
        p, q, bias = _f32c(p), _f32c(q), _f32c(bias)
        fwd = graph.fwd
        n, nnz = fwd.n_rows, fwd.nnz
        csr = fwd.device_csr()
        dev = p.device
        m, vals = (torch.empty(nnz, dtype=torch.float32, device=dev) for _ in range(2))
        s, dinv, l0_row = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        l0 = torch.empty((), dtype=torch.float32, device=dev)
        lr, n_long = _long(csr)
        rc = _lib.load().sslrec_edge_gate_fwd_f32(csr['rowptr'].data_ptr(), csr['col'].data_ptr(), csr['perm'].data_ptr(),
                                                  csr['row_of_entry'].data_ptr(), n, nnz, lr, n_long, p.data_ptr(), q.data_ptr(), bias.data_ptr(),
                                                  _ptr(noise) or None, gamma, zeta, beta, eps, m.data_ptr(), s.data_ptr(), dinv.data_ptr(),
                                                  vals.data_ptr(), l0.data_ptr(), l0_row.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_edge_gate_fwd_f32')
        ctx.graph, ctx.args, ctx.has_noise = graph, (gamma, zeta, beta, eps), noise is not None
        ctx.save_for_backward(p, q, bias, m, s, dinv, *([noise] if noise is not None else []))
        return vals, l0

    @staticmethod
    def backward(ctx, dvals, dl0):
        saved = ctx.saved_tensors
        p, q, bias, m, s, dinv = saved[:6]
        noise = saved[6] if ctx.has_noise else None
        graph = ctx.graph
        gamma, zeta, beta, eps = ctx.args
        fwd, bwd = graph.fwd, graph.bwd
        n, nnz = fwd.n_rows, fwd.nnz
        dev = p.device
        dvals = torch.zeros(nnz, dtype=torch.float32, device=dev) if dvals is None else _entry_vec(dvals, nnz, 'edge_gate backward')
        dl0 = torch.zeros((), dtype=torch.float32, device=dev) if dl0 is None else _f32c(dl0)
        cf, cb = fwd.device_csr(), bwd.device_csr()
        dp, dq = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        dbias = torch.empty_like(bias)
        dla = torch.empty(nnz, dtype=torch.float32, device=dev)
        n_ws = torch.empty(2 * n, dtype=torch.float32, device=dev)
        lr, n_long = _long(cf)
        lr_t, n_long_t = _long(cb)
        rc = _lib.load().sslrec_edge_gate_bwd_f32(cf['rowptr'].data_ptr(), cf['col'].data_ptr(), cf['perm'].data_ptr(), lr, n_long,
                                                  cb['rowptr'].data_ptr(), cb['col'].data_ptr(), cb['perm'].data_ptr(), lr_t, n_long_t, n, nnz,
                                                  p.data_ptr(), q.data_ptr(), bias.data_ptr(), _ptr(noise) or None, gamma, zeta, beta, eps,
                                                  m.data_ptr(), s.data_ptr(), dinv.data_ptr(), dvals.data_ptr(), dl0.data_ptr(), dp.data_ptr(),
                                                  dq.data_ptr(), dbias.data_ptr(), dla.data_ptr(), n_ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_edge_gate_bwd_f32')
        return dp, dq, dbias, None, None, None, None, None, None


def edge_gate(adj, p, q, bias, gamma, zeta, beta=1.0, noise=None, eps=0.0):
    """(vals [nnz], l0) of DenoiseNet's hard-concrete edge gate and symmetric normalisation (adagcl.py:274-338, :358-401, :340-347) on the
    square pattern of `adj` from the NODE vectors p, q [N] and the one-element `bias`: log_alpha[e] = p[row(e)] + q[col(e)] + bias,
    m = clamp(sigmoid(g) * (zeta - gamma) + gamma, 0, 1) with g = (noise[e] + log_alpha[e]) / beta when the logistic noise
    log u - log(1 - u) (fp32 [nnz], the caller's entry order) is given and g = log_alpha[e] otherwise, s[n] = eps + row sum of m,
    dinv = clamp(s^-0.5, 0, 10) (a row whose gates are all 0 gives inf -> 10 at eps = 0), vals[e] = m[e] dinv[row] dinv[col] -- ROW sums
    for both ends, as the reference has them -- and l0 = mean_e sigmoid(log_alpha[e] - beta log(-gamma / zeta)).  Differentiable in p, q
    and bias; the autograd node saves [nnz] and [N] vectors only, has no float atomics and gives the same bits on every run."""
    _need_gpu(p, q, bias, noise)
    graph = _pattern_graph(adj, 'edge_gate', p.device)
    if graph.bwd is None:
        raise ValueError('edge_gate: the graph needs its transposed plan')
    n_rows, n_cols = graph.shape
    gamma, zeta, beta, eps = float(gamma), float(zeta), float(beta), float(eps)
    if n_rows != n_cols or p.dim() != 1 or q.dim() != 1 or p.numel() != n_rows or q.numel() != n_rows or bias.numel() != 1:
        raise ValueError('edge_gate: p %s, q %s, bias [%d] for a %d x %d pattern' % (tuple(p.shape), tuple(q.shape), bias.numel(), n_rows, n_cols))
    if not (gamma < 0.0 < zeta and beta > 0.0 and eps >= 0.0):
        raise ValueError('edge_gate: gamma < 0 < zeta, beta > 0 and eps >= 0 expected, got %r, %r, %r, %r' % (gamma, zeta, beta, eps))
    if graph.nnz == 0 or n_rows == 0:
        raise ValueError('edge_gate: the pattern has no entries')
    if noise is not None:
        noise = _entry_vec(noise.detach(), graph.nnz, 'edge_gate noise')
    if not EDGE_GATE_FUSED:
        return _edge_gate_composed(graph.fwd.device_csr(), n_rows, p.float(), q.float(), bias.float().reshape(()), gamma, zeta, beta, noise, eps)
    return _EdgeGateFn.apply(p.float(), q.float(), bias.float().reshape(1), noise, graph, gamma, zeta, beta, eps)


# ----------------------------------------------------------------------------------------------
# fused L-layer propagation + layer SUM (+ optional per-layer perturbation)
#   S = E0 + sum_l E_l,  E_l = P_l(A E_{l-1})      (lightgcn.py:31-43 / simgcl.py:20-30)
# backward:  g_L = G,  g_{l-1} = G + A^T g_l,  dE0 = g_0   (perturbation has unit Jacobian a.e.)
# ----------------------------------------------------------------------------------------------
class RowBits:
    """Bitmap over the rows of a table: bit clear = the row is all zeros (sslrec_row_bits3).  `max_rows` = how many bits can be set."""

    def __init__(self, bits, n_rows, max_rows):
        self.bits, self.n_rows, self.max_rows = bits, int(n_rows), int(max_rows)

    @classmethod
    def from_indices(cls, n_rows, idx0, off0=0, idx1=None, off1=0, idx2=None, off2=0):
        if n_rows > (1 << 20):
            return None
        bits = torch.empty((n_rows + 31) // 32, dtype=torch.int32, device=idx0.device)
        _lib.check(_lib.load().sslrec_row_bits3(idx0.data_ptr(), int(off0), _ptr(idx1), int(off1), _ptr(idx2), int(off2), int(idx0.numel()),
                                                int(n_rows), bits.data_ptr(), _stream()), 'sslrec_row_bits3')
        k = int(idx0.numel()) * (1 + (idx1 is not None) + (idx2 is not None))
        return cls(bits, n_rows, min(n_rows, k))


SPARSE_GRAD = os.environ.get('SSLREC_SPARSE_GRAD', '1') != '0'      # the fused BPR backward tells the propagation which rows it wrote


def _tag_row_bits(t, rb):
    """remember on the tensor OBJECT which of its rows can be non-zero; valid while nobody writes to it (version counter)"""
    if rb is not None:
        t._sslrec_row_bits = (rb, t._version)


def _row_bits_of(t):
    tag = getattr(t, '_sslrec_row_bits', None)
    if tag is None or tag[1] != t._version or tag[0].n_rows != t.shape[0]:
        return None
    return tag[0]


class _PropagateSumFn(torch.autograd.Function):
    """outputs: (total, [reg], [layer 1 .. layer L]).  reg_weight (optional) adds `reg = reg_weight * sum(e0^2)` (reg_params,
    loss_utils.py:20-24) as a second output whose gradient 2 * reg_weight * g_reg * e0 is folded into the epilogue of the
    LAST backward product -- the step then needs neither a pass of its own over the table for it nor an elementwise add."""

    @staticmethod
    def forward(ctx, e0, adj, layer_num, noises, eps, keep_layers, noise_sumsq, noise_geom, reg_weight):
        ctx.adj, ctx.layer_num, ctx.reg_weight = adj, layer_num, reg_weight
        e0 = _f32c(e0)
        # deferred layer sum: the launches l < L write E_l only, the last one forms ((E0 + E1) + ...) + E_L -- the running sum's bits
        # without its 2 (L - 1) table-sized writes and L - 1 reads (column-swept layouts; L - 1 tables fit sslrec_epilogue_t.sum_in)
        plan_f = (adj.graph if isinstance(adj, (DroppedView, RevaluedView)) else adj).fwd
        lay_f = plan_f.swept(e0.shape[1]) if DEFERRED_SUM and 2 <= layer_num <= MAX_SUM_IN + 1 else None
        deferred = lay_f is not None and bool(_lib.load().sslrec_swept_deferred_sum_ok(C.byref(lay_f.c_struct())))
        reg, reg_ride = (), None
        if reg_weight is not None:
            lib = _lib.load()
            ws = _ticket_ws(e0.device, lib.sslrec_sumsq_ws_bytes(), 'sumsq')
            out = torch.empty(1, dtype=torch.float32, device=e0.device)
            # the regularizer rides on the first product (acc_out = E0 + A.E0 reads every row of E0 once in its flush) where that launch
            # is the plain one-pass swept product with a running sum; every other case keeps the launch of its own
            lay_r = None
            if (REG_IN_FLUSH and layer_num >= 1 and noises is None and not keep_layers and noise_sumsq is None and noise_geom is None
                    and not deferred):
                lay_r = plan_f.swept(e0.shape[1])
            if lay_r is not None and lay_r.n_pass == 1 and lib.sslrec_swept_step_ok(C.byref(lay_r.c_struct())):
                reg_ride = (ws, out, float(reg_weight))
                REG_ROUTES['flush'] += 1
            else:
                _lib.check(lib.sslrec_sumsq_fwd_f32(e0.data_ptr(), e0.numel(), float(reg_weight), ws.data_ptr(), out.data_ptr(), _stream()),
                           'sslrec_sumsq_fwd_f32')
                REG_ROUTES['kernel'] += 1
            reg = (out.reshape(()),)
            ctx.save_for_backward(e0)
        layers = [e0] if keep_layers else None
        ctx.row_scale = None
        if layer_num == 0:
            return (e0.clone(),) + reg
        total = torch.empty_like(e0)
        x = e0
        # factorized normalization: launch 1 reads the values and writes the SCALED table r (.) E_1, the others add rows of the scaled
        # table (no value stream) and scale the row sum in their flush
        rsc = None if (deferred or keep_layers or noise_sumsq is not None or noise_geom is not None) else \
            _chain_scale(adj, e0.shape[1], layer_num, perturbed=noises is not None)
        ctx.row_scale = rsc
        mids = []
        for l in range(layer_num):
            last = (l == layer_num - 1)
            want_y = (not last) or keep_layers
            nz = None if noises is None else noises[l]
            nss = None if noise_sumsq is None else noise_sumsq[l]
            if deferred and not last:
                y = spmm_raw(adj, x, 'fwd', noise=nz, eps=eps, noise_sumsq=nss, noise_geom=noise_geom)
                mids.append(y)
            elif deferred:
                y = spmm_raw(adj, x, 'fwd', noise=nz, eps=eps, acc_in=e0, acc_out=total, want_y=want_y, sum_in=mids,
                             noise_sumsq=nss, noise_geom=noise_geom)
            else:
                y = spmm_raw(adj, x, 'fwd', noise=nz, eps=eps, acc_in=e0 if l == 0 else total, acc_out=total, want_y=want_y,
                             chained=l > 0, noise_sumsq=nss, noise_geom=noise_geom, row_scale=rsc,
                             scale_flags=0 if rsc is None else ((SCALE_PATTERN if l > 0 else 0) | (SCALE_Y if want_y else 0)),
                             reg_sumsq=reg_ride if l == 0 else None)
            if keep_layers:
                layers.append(y)
            x = y
        ctx.mark_non_differentiable(*(layers[1:] if keep_layers else []))
        return (total,) + reg + (tuple(layers[1:]) if keep_layers else ())

    @staticmethod
    def backward(ctx, g_total, *rest):
        g_reg = rest[0] if ctx.reg_weight is not None else None
        e0 = ctx.saved_tensors[0] if ctx.reg_weight is not None else None
        if g_total is None:                 # only the regularizer was used
            return (None if g_reg is None else 2.0 * ctx.reg_weight * g_reg * e0,) + (None,) * 8
        sparse = _row_bits_of(g_total) if SPARSE_GRAD else None      # (before any copy: the tag lives on the tensor object autograd handed over)
        g_total = _f32c(g_total)
        if ctx.layer_num == 0:
            g = g_total if g_reg is None else g_total + 2.0 * ctx.reg_weight * g_reg * e0
            return (g,) + (None,) * 8
        g = g_total
        for l in range(ctx.layer_num):
            nxt = torch.empty_like(g_total)
            last = l == ctx.layer_num - 1
            rsc = ctx.row_scale      # (symmetric factors: A^T's row factor is A's)
            spmm_raw(ctx.adj, g, 'bwd', acc_in=g_total, acc_out=nxt, want_y=False, chained=l > 0,
                     axpy=(e0, 2.0 * ctx.reg_weight, g_reg) if (last and g_reg is not None) else None,
                     x_row_bits=sparse if l == 0 else None,      # A^T g: only the rows the loss wrote are gathered
                     row_scale=rsc, scale_flags=0 if rsc is None else ((SCALE_PATTERN if l > 0 else 0) | (0 if last else SCALE_ACC)))
            g = nxt
        return (g,) + (None,) * 8


def propagate_sum(adj, e0, layer_num, noises=None, eps=0.0, return_layers=False, noise_sumsq=None, noise_geom=None, reg_weight=None):
    """Sum over layers 0..L of the propagated embeddings, one fused kernel per layer.  With return_layers the per-layer
    tables come back too, for INSPECTION only: they are marked non-differentiable (the fused backward only propagates
    the gradient of the sum) -- a loss built on an individual layer must use ops.spmm per layer instead.
    reg_weight: also return `reg_weight * sum(e0^2)` (reg_params of the stacked table) -> (total, reg[, layers]); its gradient
    rides on the last backward product.  noise_sumsq (list of L [N] tensors) / noise_geom = (d_full, first column): the
    perturbation of a COLUMN SLICE of the tables (feature-sliced tables; see spmm_raw)."""
    d = e0.shape[1]
    adj = _as_adj(adj)
    dp = _spmm_dim(adj, d)
    if dp != d and noises is not None:
        if noise_geom is not None:
            raise ValueError('a column slice of %d columns is not a width of the kernels' % d)
        noises = [_pad_cols(n if torch.is_tensor(n) else n.materialize(), dp) for n in noises]
    out = _PropagateSumFn.apply(_pad_cols(e0, dp), adj, int(layer_num), noises, float(eps), bool(return_layers),
                                noise_sumsq, noise_geom, None if reg_weight is None else float(reg_weight))
    total, rest = out[0], list(out[1:])
    if dp != d:
        total = total[:, :d]
    res = [total]
    if reg_weight is not None:
        res.append(rest.pop(0))
    if return_layers:
        res.append([e0] + [l if dp == d else l[:, :d] for l in rest])
    return res[0] if len(res) == 1 else tuple(res)


def row_sumsq(x):
    """[N] sums of squares of the rows of a [N, w] table (a rank's share of EmbedPerturb's full-row noise norm, aug_utils.py:130)"""
    _need_gpu(x)
    x = _f32c(x)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().sslrec_row_sumsq_f32(x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), _stream()), 'sslrec_row_sumsq_f32')
    return out


def philox_row_sumsq(token):
    """[N] squared norms of the rows of a computed noise table (rng.PhiloxNoise over the FULL [N, d] table): what a launch on a
    column slice of that table needs beside its own columns' draws"""
    n, d = token.shape
    out = torch.empty(n, dtype=torch.float32, device=token.state.state.device)
    _lib.check(_lib.load().sslrec_philox_row_sumsq(token.state.state.data_ptr(), int(token.stream), n, d, out.data_ptr(), _stream()),
               'sslrec_philox_row_sumsq')
    return out


class _PropagateSumViewsFn(torch.autograd.Function):
    """K views of the layer-summed propagation of the SAME table over the SAME (undropped) adjacency, differing only
    in their per-layer perturbation noise (None = clean view): SimGCL's three forwards (simgcl.py:29-31).  The first
    layer is one product A.E0 with K epilogues, and the backward pass -- the same linear map for every view -- runs once, on the
    SUM of the views' upstream gradients: K - 1 + (K - 1)(L - 1) SpMM launches fewer per step, same mathematics."""

    @staticmethod
    def forward(ctx, e0, graph, layer_num, noises_views, eps):
        e0 = _f32c(e0)
        K = len(noises_views)
        ctx.graph, ctx.layer_num, ctx.K = graph, layer_num, K
        n, d = e0.shape
        lay = graph.fwd.swept(d)
        totals = [torch.empty_like(e0) for _ in range(K)]
        xs = [torch.empty_like(e0) if layer_num > 1 else None for _ in range(K)]
        rsc = _chain_scale(graph, d, layer_num, perturbed=any(nz is not None for nz in noises_views))
        ctx.row_scale = rsc
        v = _lib.EpilogueViewsStruct()
        v.n_views, v.eps = K, float(eps)
        if rsc is not None:
            v.row_scale, v.scale_flags = rsc.data_ptr(), SCALE_Y
        keep_alive = []
        for k in range(K):
            nz = None if noises_views[k] is None else noises_views[k][0]
            if nz is not None and not torch.is_tensor(nz):            # rng.PhiloxNoise
                v.philox, v.philox_stream[k], v.philox_noise[k] = nz.state.state.data_ptr(), int(nz.stream), 1
                nz = None
            elif nz is not None:
                nz = _f32c(nz)
            keep_alive.append(nz)
            v.Y[k] = _ptr(xs[k]) or None
            v.noise[k] = _ptr(nz) or None
            v.acc_in[k] = e0.data_ptr()
            v.acc_out[k] = totals[k].data_ptr()
        ev0 = ev1 = None
        if _profile_this_launch():      # (the same sampling tick as every other SpMM launch: the sampled launch rotates through ALL of a step's)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        rc = _lib.load().sslrec_spmm_swept_views_f32(C.byref(lay.c_struct()), e0.data_ptr(), d, C.byref(v), _stream())
        _lib.check(rc, 'sslrec_spmm_swept_views_f32')
        if PROFILE is not None:
            if ev1 is not None:
                ev1.record()
            PROFILE.append((ev0, ev1, lay, d, True, layer_num > 1, 1.0, None, 0, False,
                            {'views': K, 'perturbed': any(nz is not None for nz in noises_views),
                             'philox': any(v.philox_noise[k] for k in range(K)), 'which': 'fwd'}))
        for k in range(K):
            x = xs[k]
            for l in range(1, layer_num):
                last = (l == layer_num - 1)
                x = spmm_raw(graph, x, 'fwd', noise=None if noises_views[k] is None else noises_views[k][l], eps=eps,
                             acc_in=totals[k], acc_out=totals[k], want_y=not last, row_scale=rsc,
                             scale_flags=0 if rsc is None else (SCALE_PATTERN | (0 if last else SCALE_Y)))
        return tuple(totals)

    @staticmethod
    def backward(ctx, *g_totals):
        # The perturbation adds eps * sign(y) * noise / |noise| (aug_utils.py:125-132): its derivative with respect to y is the identity,
        # so every view's backward pass is the SAME linear map  g -> g + A^T (g + A^T (g + ...))  of its upstream gradient, and the sum
        # over the views of the maps is the map of the sum: L products for all K views instead of K (L - 1) + 1, and K - 1 table
        # additions instead of 2 (K - 1).  (SimGCL, K = 3, L = 2: 4 -> 2 backward products per step.)
        graph, L = ctx.graph, ctx.layer_num
        grads = [_f32c(g) for g in g_totals if g is not None]
        if not grads:
            return None, None, None, None, None
        G = grads[0]
        for i, g in enumerate(grads[1:]):
            G = torch.add(G, g) if i == 0 else G.add_(g)
        g = G
        rsc = ctx.row_scale
        for l in range(L):
            nxt = torch.empty_like(G)
            spmm_raw(graph, g, 'bwd', acc_in=G, acc_out=nxt, want_y=False, row_scale=rsc,
                     scale_flags=0 if rsc is None else ((SCALE_PATTERN if l > 0 else 0) | (0 if l == L - 1 else SCALE_ACC)))
            g = nxt
        return g, None, None, None, None


class _PropagateSumViewsLoopFn(torch.autograd.Function):
    """The same K views where the first layer's product cannot be shared (a table beyond the column-swept layout, a narrow or padded
    width, a column slice of the tables with its noise geometry): K separate forward chains, but still ONE backward chain on the
    summed upstream gradients (see _PropagateSumViewsFn.backward: the perturbation's derivative is the identity)."""

    @staticmethod
    def forward(ctx, e0, adj, layer_num, noises_views, eps, sumsq_views, noise_geom):
        e0 = _f32c(e0)
        ctx.adj, ctx.layer_num = adj, layer_num
        rsc = _chain_scale(adj, e0.shape[1], layer_num, perturbed=any(nz is not None for nz in noises_views)) \
            if (sumsq_views is None and noise_geom is None) else None
        ctx.row_scale = rsc
        totals = []
        for k, nzs in enumerate(noises_views):
            total = torch.empty_like(e0)
            x = e0
            for l in range(layer_num):
                last = (l == layer_num - 1)
                x = spmm_raw(adj, x, 'fwd', noise=None if nzs is None else nzs[l], eps=eps, acc_in=e0 if l == 0 else total, acc_out=total,
                             want_y=not last, noise_sumsq=None if (nzs is None or sumsq_views is None or sumsq_views[k] is None) else sumsq_views[k][l],
                             noise_geom=None if nzs is None else noise_geom, row_scale=rsc,
                             scale_flags=0 if rsc is None else ((SCALE_PATTERN if l > 0 else 0) | (0 if last else SCALE_Y)))
            totals.append(total)
        return tuple(totals)

    @staticmethod
    def backward(ctx, *g_totals):
        grads = [_f32c(g) for g in g_totals if g is not None]
        if not grads:
            return (None,) * 7
        G = grads[0]
        for i, g in enumerate(grads[1:]):
            G = torch.add(G, g) if i == 0 else G.add_(g)
        g = G
        rsc, L = ctx.row_scale, ctx.layer_num
        for l in range(L):
            nxt = torch.empty_like(G)
            spmm_raw(ctx.adj, g, 'bwd', acc_in=G, acc_out=nxt, want_y=False, row_scale=rsc,
                     scale_flags=0 if rsc is None else ((SCALE_PATTERN if l > 0 else 0) | (0 if l == L - 1 else SCALE_ACC)))
            g = nxt
        return (g,) + (None,) * 6


def propagate_sum_views(adj, e0, layer_num, noises_views, eps=0.0, noise_sumsq_views=None, noise_geom=None):
    """[propagate_sum(adj, e0, L, noises_k, eps) for noises_k in noises_views] -- views of the SAME table over the SAME adjacency that
    differ only in their perturbation noise (None = the clean view) -- with ONE backward chain for all views and, on the column-swept
    layout of the plain graph, the first layer's product shared too (K epilogues).  noise_sumsq_views (per view: L [N] tensors, or
    None) / noise_geom: the perturbation of a COLUMN SLICE of the tables (see propagate_sum)."""
    adj = _as_adj(adj)
    d = e0.shape[1]
    if layer_num < 1 or len(noises_views) < 2:
        return [propagate_sum(adj, e0, layer_num, nz, eps, noise_sumsq=None if noise_sumsq_views is None else noise_sumsq_views[k],
                              noise_geom=None if nz is None else noise_geom) for k, nz in enumerate(noises_views)]
    shared = (isinstance(adj, PropGraph) and d in SPMM_DIMS and len(noises_views) <= 4 and noise_sumsq_views is None and noise_geom is None
              and adj.bwd is not None and adj.fwd.swept(d) is not None)
    if shared:
        return list(_PropagateSumViewsFn.apply(e0, adj, int(layer_num), list(noises_views), float(eps)))
    dp = _spmm_dim(adj, d)
    if dp != d:
        if noise_geom is not None:
            raise ValueError('a column slice of %d columns is not a width of the kernels' % d)
        noises_views = [None if nzs is None else [_pad_cols(n if torch.is_tensor(n) else n.materialize(), dp) for n in nzs] for nzs in noises_views]
    outs = _PropagateSumViewsLoopFn.apply(_pad_cols(e0, dp), adj, int(layer_num), list(noises_views), float(eps), noise_sumsq_views, noise_geom)
    return [t if dp == d else t[:, :d] for t in outs]


# ----------------------------------------------------------------------------------------------
# BPR
# ----------------------------------------------------------------------------------------------
class _BprFn(torch.autograd.Function):
    """loss = sum_b f(<a,n> - <a,p>) over rows gathered from up to three tables."""

    @staticmethod
    def forward(ctx, ta, tp, tn, ia, ip, in_, variant, shared_pn, divisor=1.0):
        _need_gpu(ta, tp, tn)
        ta, tp, tn = _f32c(ta), _f32c(tp), _f32c(tn)
        ia, ip, in_ = _idx(ia), _idx(ip), _idx(in_)
        B = int(ia.numel()) if ia is not None else ta.shape[0]
        d = ta.shape[1]
        lib = _lib.load()
        ws = _ticket_ws(ta.device, lib.sslrec_bpr_ws_bytes(B), 'bpr')
        out = torch.empty(1, dtype=torch.float32, device=ta.device)
        rc = lib.sslrec_bpr_fwd_f32(ta.data_ptr(), _ptr(ia), tp.data_ptr(), _ptr(ip), tn.data_ptr(), _ptr(in_), B, d,
                                    variant, float(divisor), ws.data_ptr(), out.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_bpr_fwd_f32')
        ctx.save_for_backward(ta, tp, tn, ia if ia is not None else torch.empty(0), ip if ip is not None else torch.empty(0),
                              in_ if in_ is not None else torch.empty(0))
        ctx.has_idx = (ia is not None, ip is not None, in_ is not None)
        ctx.meta = (B, d, variant, shared_pn, float(divisor))
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        ta, tp, tn, ia, ip, in_ = ctx.saved_tensors
        ia = ia if ctx.has_idx[0] else None
        ip = ip if ctx.has_idx[1] else None
        in_ = in_ if ctx.has_idx[2] else None
        B, d, variant, shared_pn, divisor = ctx.meta
        g = g.reshape(1).to(torch.float32).contiguous()
        dta = torch.zeros_like(ta) if ia is not None else torch.empty_like(ta)
        if shared_pn:                       # positives and negatives index the SAME table
            dtp = torch.zeros_like(tp)
            dtn = dtp
        else:
            dtp = torch.zeros_like(tp) if ip is not None else torch.empty_like(tp)
            dtn = torch.zeros_like(tn) if in_ is not None else torch.empty_like(tn)
        lib = _lib.load()
        ws, kept = _bpr_bwd_ws(ta.device, B, d)
        args = (ta.data_ptr(), _ptr(ia), tp.data_ptr(), _ptr(ip), tn.data_ptr(), _ptr(in_), B, d,
                variant, divisor, g.data_ptr(), dta.data_ptr(), dtp.data_ptr(), dtn.data_ptr(), ws.data_ptr())
        rc = lib.sslrec_bpr_bwd_kept_f32(*args, None, 0, _stream()) if kept else lib.sslrec_bpr_bwd_f32(*args, _stream())
        _check_kept(rc, 'sslrec_bpr_bwd_f32', ta.device, B, d)
        return dta, dtp, (None if shared_pn else dtn), None, None, None, None, None, None


def bpr_loss_and_grads(anc, pos, neg, variant=0, divisor=1.0):
    """cal_bpr_loss(anc, pos, neg) / divisor (loss_utils.py:7-10) and its gradients w.r.t. the three dense [B, d] operands in
    two launches, WITHOUT autograd: the building block of a hand-written backward pass (sslrec_amd/feature_shard.py's captured
    step).  Returns (loss [1], d_anc, d_pos, d_neg)."""
    _need_gpu(anc, pos, neg)
    anc, pos, neg = _f32c(anc.detach()), _f32c(pos.detach()), _f32c(neg.detach())
    B, d = anc.shape
    lib = _lib.load()
    dev = anc.device
    ws = _ticket_ws(dev, lib.sslrec_bpr_ws_bytes(B), 'bpr')
    out = torch.empty(1, dtype=torch.float32, device=dev)
    rc = lib.sslrec_bpr_fwd_f32(anc.data_ptr(), None, pos.data_ptr(), None, neg.data_ptr(), None, B, d, int(variant),
                                float(divisor), ws.data_ptr(), out.data_ptr(), _stream())
    _lib.check(rc, 'sslrec_bpr_fwd_f32')
    one = torch.ones(1, dtype=torch.float32, device=dev)
    da, dp, dn = torch.empty_like(anc), torch.empty_like(pos), torch.empty_like(neg)
    ws2 = torch.empty(lib.sslrec_bpr_bwd_ws_bytes(B, d) // 4 + 1, dtype=torch.float32, device=dev)
    rc = lib.sslrec_bpr_bwd_f32(anc.data_ptr(), None, pos.data_ptr(), None, neg.data_ptr(), None, B, d, int(variant),
                                float(divisor), one.data_ptr(), da.data_ptr(), dp.data_ptr(), dn.data_ptr(), ws2.data_ptr(), _stream())
    _lib.check(rc, 'sslrec_bpr_bwd_f32')
    return out, da, dp, dn


def bpr_loss(anc, pos, neg, variant=0, divisor=1.0):
    """Dense drop-in for cal_bpr_loss(anc[B,d], pos[B,d], neg[B,d]) (loss_utils.py:7-10); returns the SUM, divided by
    `divisor` inside the kernel (pass the batch size to fold the reference's `/ ancs.shape[0]`)."""
    return _BprFn.apply(anc, pos, neg, None, None, None, int(variant), False, float(divisor))


class _BprStackedFn(torch.autograd.Function):
    """BPR over ONE stacked table [users; items]: anchors index its first n_user rows, positives / negatives the rows
    after them (the item part is addressed through an offset base pointer -- no index arithmetic); one gradient buffer.
    With `add` (a 0-d tensor, e.g. the regularizer term) the SAME launch also returns total = bpr + add (lightgcn.py:54's
    `bpr_loss + reg_loss`): outputs (total, bpr), the gradient of `total` flows to the table and, unchanged, to `add`."""

    @staticmethod
    def forward(ctx, table, n_user, ancs, poss, negs, variant, divisor, add, stage):
        _need_gpu(table)
        table = _f32c(table)
        ia, ip, in_ = _idx(ancs), _idx(poss), _idx(negs)
        B, d = int(ia.numel()), table.shape[1]
        lib = _lib.load()
        ws = _ticket_ws(table.device, lib.sslrec_bpr_ws_bytes(B), 'bpr')
        p = table.data_ptr()
        pi = p + int(n_user) * d * 4
        ctx.save_for_backward(table, ia, ip, in_)
        ctx.meta = (B, d, variant, int(n_user), float(divisor))
        ctx.two = add is not None
        ctx.staged = None
        ctx.set_materialize_grads(False)
        if stage and SSLREC_KEPT_SCATTER and 0 < 3 * B <= 16384 and d <= 256 and table.numel() % 4 == 0:
            # the backward is known to follow: this launch also stages its rows (for an upstream gradient of 1), registers their
            # destinations in the kept workspace and zeroes the gradient table; the backward is then the reduction alone.  The
            # workspace is shared per (device, B, d): the record's generation tells the backward whether the rows are still its own.
            if add is not None:
                _need_gpu(add)
            addc = None if add is None else add.detach().reshape(1).to(torch.float32).contiguous()
            out = torch.empty(1 if add is None else 2, dtype=torch.float32, device=table.device)
            wsb, _ = _bpr_bwd_ws(table.device, B, d)      # (clears the table first if an earlier staging was never consumed)
            grad = torch.empty_like(table)
            q = grad.data_ptr()
            qi = q + int(n_user) * d * 4
            rc = lib.sslrec_bpr_fwd_staged_f32(p, ia.data_ptr(), pi, ip.data_ptr(), pi, in_.data_ptr(), B, d, variant, float(divisor),
                                               _ptr(addc), ws.data_ptr(), out.data_ptr(), q, qi, qi, wsb.data_ptr(), q, grad.numel(),
                                               _stream())
            _check_kept(rc, 'sslrec_bpr_fwd_staged_f32', table.device, B, d)
            st = wsb._sslrec_stage
            st[0], st[1] = st[0] + 1, True
            ctx.staged = (wsb, st[0], grad)
            return out.reshape(()) if add is None else (out[1].reshape(()), out[0].reshape(()))
        if add is None:
            out = torch.empty(1, dtype=torch.float32, device=table.device)
            rc = lib.sslrec_bpr_fwd_f32(p, ia.data_ptr(), pi, ip.data_ptr(), pi, in_.data_ptr(), B, d, variant, float(divisor),
                                        ws.data_ptr(), out.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_bpr_fwd_f32')
            return out.reshape(())
        _need_gpu(add)
        addc = add.detach().reshape(1).to(torch.float32).contiguous()
        out = torch.empty(2, dtype=torch.float32, device=table.device)
        rc = lib.sslrec_bpr_fwd_total_f32(p, ia.data_ptr(), pi, ip.data_ptr(), pi, in_.data_ptr(), B, d, variant, float(divisor),
                                          addc.data_ptr(), ws.data_ptr(), out.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_bpr_fwd_total_f32')
        return out[1].reshape(()), out[0].reshape(())

    @staticmethod
    def backward(ctx, *grads):
        table, ia, ip, in_ = ctx.saved_tensors
        B, d, variant, n_user, divisor = ctx.meta
        if ctx.two:                  # outputs (total, bpr): total's gradient goes to the table AND to `add`; bpr's (if anybody
            g_total, g_bpr = grads   # differentiates the logged part too) to the table only
            g_add = g_total
            g = g_total if g_bpr is None else (g_bpr if g_total is None else g_total + g_bpr)
        else:
            g, g_add = grads[0], None
        if g is None:
            return None, None, None, None, None, None, None, g_add, None
        g = g.reshape(1).to(torch.float32).contiguous()
        lib = _lib.load()
        staged, ctx.staged = ctx.staged, None      # (a second backward under retain_graph takes the three-launch form below)
        if staged is not None:
            wsb, gen, grad = staged
            if _kept_ws(table.device, B, d) is wsb and wsb._sslrec_stage == [gen, True]:      # nobody has used the workspace since
                wsb._sslrec_stage[1] = False
                rc = lib.sslrec_bpr_bwd_from_staged_f32(B, d, g.data_ptr(), wsb.data_ptr(), _stream())
                _check_kept(rc, 'sslrec_bpr_bwd_from_staged_f32', table.device, B, d)
                if SPARSE_GRAD:
                    _tag_row_bits(grad, RowBits.from_indices(table.shape[0], ia, 0, ip, n_user, in_, n_user))
                return grad, None, None, None, None, None, None, g_add, None
        ws, kept = _bpr_bwd_ws(table.device, B, d)
        fused_zero = kept and B > 0 and table.numel() % 4 == 0      # the staging launch zeroes the gradient table itself: no fill launch
        grad = torch.empty_like(table) if fused_zero else torch.zeros_like(table)
        p, q = table.data_ptr(), grad.data_ptr()
        pi, qi = p + n_user * d * 4, q + n_user * d * 4
        args = (p, ia.data_ptr(), pi, ip.data_ptr(), pi, in_.data_ptr(), B, d, variant, divisor, g.data_ptr(), q, qi, qi, ws.data_ptr())
        if kept:
            rc = lib.sslrec_bpr_bwd_kept_f32(*args, q if fused_zero else None, grad.numel() if fused_zero else 0, _stream())
        else:
            rc = lib.sslrec_bpr_bwd_f32(*args, _stream())
        _check_kept(rc, 'sslrec_bpr_bwd_f32', table.device, B, d)
        if SPARSE_GRAD:      # rows ancs / n_user + poss / n_user + negs are the only ones written
            _tag_row_bits(grad, RowBits.from_indices(table.shape[0], ia, 0, ip, n_user, in_, n_user))
        return grad, None, None, None, None, None, None, g_add, None


def bpr_loss_stacked(table, n_user, ancs, poss, negs, variant=0, divisor=1.0, add=None):
    """Fused gather + BPR on the stacked [users; items] table the propagation produces (no slicing,
    one [N, d] gradient buffer): rows ancs / n_user + poss / n_user + negs (lightgcn.py:49-52).
    add (0-d tensor): returns (bpr + add, bpr) from the same launch."""
    # (grad mode is off inside Function.forward: whether a backward can follow is decided here.  A forward under no_grad, or on a table
    # that takes no gradient, stages nothing and costs what it did)
    stage = BPR_STAGED and torch.is_grad_enabled() and table.requires_grad
    return _BprStackedFn.apply(table, int(n_user), ancs, poss, negs, int(variant), float(divisor), add, stage)


def bpr_loss_gathered(user_table, item_table, ancs, poss, negs, variant=0, divisor=1.0):
    """Fused gather + BPR: rows user_table[ancs], item_table[poss], item_table[negs]
    (lightgcn.py:49-52) without materializing the three [B,d] gathers."""
    return _BprFn.apply(user_table, item_table, item_table, ancs, poss, negs, int(variant), True, float(divisor))


# ----------------------------------------------------------------------------------------------
# InfoNCE
# ----------------------------------------------------------------------------------------------
def _infonce_event():
    if PROFILE_INFONCE is None:
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


def _infonce_record(ev0, kind, B, M, d, variant):
    if ev0 is not None and PROFILE_INFONCE is not None:
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        PROFILE_INFONCE.append((ev0, ev1, kind, B, M, d, variant))


def infonce_issued_flops(kind, B, M, d, variant):
    """matrix-core work ONE call issues, as (flops, 'bf16' | 'fp32'): a B x M x d product is 2BMd flops in exact-fp32 MFMA and
    (planes-dependent) 3 or 6 bf16 MFMA terms of 2BMd each in the split-precision modes (csrc/infonce_x3.inc).  Forward = the
    scores (+ the anchor-gradient product under SSLREC_INFONCE_FWD_W); backward = scores + the `all`-gradient product (+ scores and
    the anchor-gradient product again without the flag)."""
    code = (variant >> 8) & 0xFF
    v1 = (variant & 0xFF) != 0
    if code == 0:      # the library's defaults (csrc/infonce.hip, inf_precision): h3 -- on the un-normalized variant unless SSLREC_INFONCE_V1_DEFAULT=x6
        v1_default = 'x6' if (os.environ.get('SSLREC_INFONCE_V1_DEFAULT') or 'h3')[0] == 'x' else 'h3'
        code = INFONCE_PRECISIONS.get(os.environ.get('SSLREC_INFONCE_PRECISION') or (v1_default if v1 else 'h3'), 1)
    if v1 and code not in (2, 7):      # un-normalized rows: x6, exact fp32, or h3 with device-chosen scales; the other modes run x6
        code = 1
    fwd_w = bool(variant & INFONCE_FWD_W_BIT) and not (code == 2 and d == 128)
    # terms per (score product, anchor-gradient product, all-gradient product)
    sc, wa, da = {1: (6, 6, 6), 2: (1, 1, 1), 3: (3, 6, 6), 4: (3, 3, 3), 5: (6, 3, 3), 6: (6, 6, 3), 7: (3, 3, 3)}[code]
    unit = 2.0 * B * M * d
    pre = 1 if (v1 and code == 7 and (kind == 'fwd')) else 0      # h3 on the un-normalized variant: the row-max pre-pass, one term on the high planes
    if kind == 'fwd':
        f = sc + (wa if fwd_w else 0) + pre
    else:
        f = sc + da + (0 if fwd_w else sc + wa)
    return f * unit, ('fp32' if code == 2 else ('fp16' if code == 7 else 'bf16'))


class _InfoNceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t1, t2, all_, i1, i2, temp, variant, t2_is_all, will_differentiate=True):
        _need_gpu(t1, t2, all_)
        t1, t2, all_ = _f32c(t1), _f32c(t2), _f32c(all_)
        i1, i2 = _idx(i1), _idx(i2)
        B = int(i1.numel()) if i1 is not None else t1.shape[0]
        M, d = all_.shape
        if d not in INFONCE_DIMS:
            raise ValueError('embedding size %d not supported by the HIP InfoNCE (supported: %s)' % (d, INFONCE_DIMS))
        lib = _lib.load()
        if INFONCE_FWD_W and will_differentiate and any(ctx.needs_input_grad[:3]):
            variant |= INFONCE_FWD_W_BIT
        ws = torch.empty(lib.sslrec_infonce_ws_bytes(B, M, d) // 4, dtype=torch.float32, device=t1.device)
        out = torch.empty(1, dtype=torch.float32, device=t1.device)
        ev = _infonce_event()
        rc = lib.sslrec_infonce_fwd_f32(t1.data_ptr(), _ptr(i1), t2.data_ptr(), _ptr(i2), B, all_.data_ptr(), M, d,
                                        float(temp), variant, ws.data_ptr(), out.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_infonce_fwd_f32')
        _infonce_record(ev, 'fwd', B, M, d, variant)
        ctx.save_for_backward(t1, t2, all_, i1 if i1 is not None else torch.empty(0),
                              i2 if i2 is not None else torch.empty(0), ws)
        ctx.has_idx = (i1 is not None, i2 is not None)
        ctx.meta = (B, M, d, float(temp), variant, t2_is_all)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        t1, t2, all_, i1, i2, ws = ctx.saved_tensors
        i1 = i1 if ctx.has_idx[0] else None
        i2 = i2 if ctx.has_idx[1] else None
        B, M, d, temp, variant, t2_is_all = ctx.meta
        g = g.reshape(1).to(torch.float32).contiguous()
        dev = t1.device
        lib = _lib.load()
        ev = _infonce_event()
        if i1 is not None and i2 is not None and 2 * B <= 16384:
            # both roles gathered (simgcl.py:49 / sgl.py:57-59): backward + one deterministic scatter for both in one call
            de = torch.empty((2 * B, d), dtype=torch.float32, device=dev)
            dall = torch.empty((M, d), dtype=torch.float32, device=dev)
            dt1 = torch.zeros_like(t1)
            dt2 = dall if t2_is_all else torch.zeros_like(t2)
            sws = torch.empty(lib.sslrec_scatter_ws_bytes(2 * B) // 4 + 1, dtype=torch.float32, device=dev)
            rc = lib.sslrec_infonce_bwd_scatter_f32(t1.data_ptr(), i1.data_ptr(), t2.data_ptr(), i2.data_ptr(), B, all_.data_ptr(), M, d,
                                                    temp, variant, ws.data_ptr(), g.data_ptr(), de.data_ptr(), dt1.data_ptr(),
                                                    dt2.data_ptr(), dall.data_ptr(), sws.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_infonce_bwd_scatter_f32')
            _infonce_record(ev, 'bwd', B, M, d, variant)
            return (dt1, None, dall, None, None, None, None, None, None) if t2_is_all else (dt1, dt2, dall, None, None, None, None, None, None)
        de1 = torch.empty((B, d), dtype=torch.float32, device=dev)
        de2 = torch.empty((B, d), dtype=torch.float32, device=dev)
        dall = torch.empty((M, d), dtype=torch.float32, device=dev)
        rc = lib.sslrec_infonce_bwd_f32(t1.data_ptr(), _ptr(i1), t2.data_ptr(), _ptr(i2), B, all_.data_ptr(), M, d,
                                        temp, variant, ws.data_ptr(), g.data_ptr(), de1.data_ptr(), de2.data_ptr(),
                                        dall.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_infonce_bwd_f32')
        _infonce_record(ev, 'bwd', B, M, d, variant)

        def scatter(src, idx, dst):
            sws = torch.empty(lib.sslrec_scatter_ws_bytes(B) // 4 + 1, dtype=torch.float32, device=src.device)
            rc2 = lib.sslrec_scatter_add_rows_f32(src.data_ptr(), idx.data_ptr(), B, d, dst.data_ptr(), sws.data_ptr(), _stream())
            _lib.check(rc2, 'sslrec_scatter_add_rows_f32')

        if i1 is not None:
            dt1 = torch.zeros_like(t1)
            scatter(de1, i1, dt1)
        else:
            dt1 = de1
        if t2_is_all:                       # e2 rows are gathered from the same table as `all`
            if i2 is not None:
                scatter(de2, i2, dall)
            else:
                dall += de2
            return dt1, None, dall, None, None, None, None, None, None
        if i2 is not None:
            dt2 = torch.zeros_like(t2)
            scatter(de2, i2, dt2)
        else:
            dt2 = de2
        return dt1, dt2, dall, None, None, None, None, None, None


def infonce_loss(embeds1, embeds2, all_embeds2, temp=1.0, variant=0, precision=None):
    """Dense drop-in for cal_infonce_loss(embeds1[B,d], embeds2[B,d], all_embeds2[M,d], temp)
    (loss_utils.py:30-39); returns the SUM over the batch.  `precision`: 'x6' | 'fp32' | 'x6a' | 'x63' | 'x36' | 'x3' | None (default)."""
    dp = _padded_dim(embeds1.shape[1], INFONCE_DIMS)
    return _InfoNceFn.apply(_pad_cols(embeds1, dp), _pad_cols(embeds2, dp), _pad_cols(all_embeds2, dp), None, None,
                            float(temp), _variant_code(variant, precision), False, torch.is_grad_enabled())


def infonce_loss_gathered(table1, table2, idx, temp=1.0, variant=0, precision=None):
    """Fused form of cal_infonce_loss(table1[idx], table2[idx], table2, temp) -- the call shape of
    simgcl.py:49 and sgl.py:57-59 -- without materializing the gathers."""
    dp = _padded_dim(table1.shape[1], INFONCE_DIMS)
    if dp != table1.shape[1]:
        table1, table2 = _pad_cols(table1, dp), _pad_cols(table2, dp)
    # (inside Function.forward grad mode is always off and needs_input_grad ignores no_grad(): the caller's grad mode is passed in)
    return _InfoNceFn.apply(table1, table2, table2, idx, idx, float(temp), _variant_code(variant, precision), True, torch.is_grad_enabled())


class _InfoNceTwoSidedFn(torch.autograd.Function):
    """cal_infonce_loss(U1[iu], U2[iu], U2, temp) + cal_infonce_loss(I1[ii], I2[ii], I2, temp) (simgcl.py:49, sgl.py:57-59) on the STACKED
    tables s = [U; I] that the propagation returns, as ONE autograd node: the gradients of both terms are written straight into one
    [N, d] buffer per view (the `all`-side gradient covers every row of view 2's buffer, so only view 1's is zero-filled).  Going
    through the split tables instead costs, per view and step, two slice-backward nodes (a table-sized zero fill + copy each) and
    the add that joins them -- ~150 us of stock elementwise launches per SimGCL step at amazon-book size (profiles/r04/cfg3_kernel_stats.csv)."""

    @staticmethod
    def forward(ctx, s1, s2, n_user, iu, ii, temp, variant, will_differentiate):
        _need_gpu(s1, s2)
        s1, s2 = _f32c(s1), _f32c(s2)
        iu, ii = _idx(iu), _idx(ii)
        N, d = s1.shape
        lib = _lib.load()
        if INFONCE_FWD_W and will_differentiate and any(ctx.needs_input_grad[:2]):
            variant |= INFONCE_FWD_W_BIT
        sides = [(0, int(n_user), iu), (int(n_user), N - int(n_user), ii)]
        outs = torch.empty(2, dtype=torch.float32, device=s1.device)
        wss = []
        for k, (row0, M, idx) in enumerate(sides):
            B = int(idx.numel())
            off = row0 * d * 4
            ws = torch.empty(lib.sslrec_infonce_ws_bytes(B, M, d) // 4, dtype=torch.float32, device=s1.device)
            ev = _infonce_event()
            rc = lib.sslrec_infonce_fwd_f32(s1.data_ptr() + off, idx.data_ptr(), s2.data_ptr() + off, idx.data_ptr(), B, s2.data_ptr() + off, M, d,
                                            float(temp), variant, ws.data_ptr(), outs.data_ptr() + 4 * k, _stream())
            _lib.check(rc, 'sslrec_infonce_fwd_f32')
            _infonce_record(ev, 'fwd', B, M, d, variant)
            wss.append(ws)
        ctx.save_for_backward(s1, s2, iu, ii, *wss)
        ctx.meta = (int(n_user), float(temp), variant)
        return outs[0] + outs[1]

    @staticmethod
    def backward(ctx, g):
        s1, s2, iu, ii, ws_u, ws_i = ctx.saved_tensors
        n_user, temp, variant = ctx.meta
        N, d = s1.shape
        g = g.reshape(1).to(torch.float32).contiguous()
        lib = _lib.load()
        g1 = torch.zeros_like(s1)             # the anchors' rows are scattered into it
        g2 = torch.empty_like(s2)             # every row is written: it is the `all` operand of one of the two terms
        for row0, M, idx, ws in ((0, n_user, iu, ws_u), (n_user, N - n_user, ii, ws_i)):
            B = int(idx.numel())
            off = row0 * d * 4
            de = torch.empty((2 * B, d), dtype=torch.float32, device=s1.device)
            sws = torch.empty(lib.sslrec_scatter_ws_bytes(2 * B) // 4 + 1, dtype=torch.float32, device=s1.device)
            ev = _infonce_event()
            rc = lib.sslrec_infonce_bwd_scatter_f32(s1.data_ptr() + off, idx.data_ptr(), s2.data_ptr() + off, idx.data_ptr(), B, s2.data_ptr() + off, M, d,
                                                    temp, variant, ws.data_ptr(), g.data_ptr(), de.data_ptr(), g1.data_ptr() + off,
                                                    g2.data_ptr() + off, g2.data_ptr() + off, sws.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_infonce_bwd_scatter_f32')
            _infonce_record(ev, 'bwd', B, M, d, variant)
        return g1, g2, None, None, None, None, None, None


def infonce_loss_two_sided(stacked1, stacked2, n_user, user_idx, item_idx, temp=1.0, variant=0, precision=None):
    """cal_infonce_loss(U1[user_idx], U2[user_idx], U2, temp) + cal_infonce_loss(I1[item_idx], I2[item_idx], I2, temp) with
    [U_k; I_k] = stacked_k -- the contrastive term of SimGCL (simgcl.py:49) and, with item_idx = [poss; negs], of SGL (sgl.py:57-59) --
    on the propagation's stacked tables, one autograd node (see _InfoNceTwoSidedFn).  Embedding sizes without a kernel width and
    batches beyond the scatter table take the two gathered calls on the split tables."""
    d = stacked1.shape[1]
    if d not in INFONCE_DIMS or 2 * max(int(user_idx.numel()), int(item_idx.numel())) > 16384 or not stacked1.is_cuda:
        return infonce_loss_gathered(stacked1[:n_user], stacked2[:n_user], user_idx, temp, variant, precision) + \
            infonce_loss_gathered(stacked1[n_user:], stacked2[n_user:], item_idx, temp, variant, precision)
    return _InfoNceTwoSidedFn.apply(stacked1, stacked2, int(n_user), user_idx, item_idx, float(temp), _variant_code(variant, precision),
                                    torch.is_grad_enabled())


# ----------------------------------------------------------------------------------------------
# alignment + uniformity loss of DirectAU (loss_utils.py:75-86, directau.py:42-47) on the stacked table: gathers, both normalisations,
# the B x B Gaussian pair sums and the index_put backward as one autograd node, nothing of size B^2 stored (csrc/au.hip)
# ----------------------------------------------------------------------------------------------
AU_DIMS = (32, 64, 128)
AU_MAX_BATCH = 8192          # 2 B gathered rows must fit the deterministic scatter's table
AU_ALIGN, AU_UNIFORM_ANC, AU_UNIFORM_POS = 1, 2, 4


def _au_uniformity(x):
    """loss_utils.py:82-86"""
    x = torch.nn.functional.normalize(x, dim=-1)
    return torch.pdist(x, p=2).pow(2).mul(-2).exp().mean().log()


def _au_alignment(x, y, alpha=2):
    """loss_utils.py:75-79"""
    x, y = torch.nn.functional.normalize(x, dim=-1), torch.nn.functional.normalize(y, dim=-1)
    return (x - y).norm(p=2, dim=1).pow(alpha).mean()


def _au_composed(table, n_user, ancs, poss, gamma, scale):
    """the reference's expression (directau.py:35, 43-47) on the layer sum"""
    anc, pos = table[:n_user][ancs] * scale, table[n_user:][poss] * scale
    align = _au_alignment(anc, pos)
    uniform = gamma * (_au_uniformity(anc) + _au_uniformity(pos)) / 2
    return align + uniform, align, uniform


class _AlignUniformFn(torch.autograd.Function):
    """outputs (loss, align_loss, uniform_loss) from one 5-float result; keeps the workspace (normalised rows, norms) for the backward,
    which recomputes the pair terms and scatters both gathers' gradients into one [N, d] buffer"""

    @staticmethod
    def forward(ctx, table, n_user, ancs, poss, gamma, scale, terms):
        table = _f32c(table)
        ia, ip = _idx(ancs), _idx(poss)
        n, d = table.shape
        B = int(ia.numel())
        lib = _lib.load()
        ws = torch.empty(lib.sslrec_au_ws_bytes(B, d) // 4 + 1, dtype=torch.float32, device=table.device)
        out = torch.empty(8, dtype=torch.float32, device=table.device)
        rc = lib.sslrec_au_fwd_f32(table.data_ptr(), n, n_user, d, ia.data_ptr(), ip.data_ptr(), B, scale, gamma, terms, out.data_ptr(),
                                   ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_au_fwd_f32')
        ctx.save_for_backward(ia, ip, out)
        ctx.ws = ws
        ctx.meta = (n, d, B, n_user, gamma, scale, terms)
        ctx.set_materialize_grads(False)
        return out[0].reshape(()), out[1].reshape(()), out[2].reshape(())

    @staticmethod
    def backward(ctx, g_loss, g_align, g_uniform):
        ia, ip, out = ctx.saved_tensors
        n, d, B, n_user, gamma, scale, terms = ctx.meta
        both = lambda a, b: a if b is None else (b if a is None else a + b)
        ga, gu = both(g_loss, g_align), both(g_loss, g_uniform)       # loss = align + uniform: the usual call has g_loss alone
        if ga is None and gu is None:
            return None, None, None, None, None, None, None
        as_dev = lambda g: torch.zeros(1, dtype=torch.float32, device=out.device) if g is None else g.reshape(1).to(torch.float32).contiguous()
        ga = as_dev(ga)
        gu = ga if gu is g_loss and g_align is None else as_dev(gu)
        grad = torch.zeros(n, d, dtype=torch.float32, device=out.device)
        lib = _lib.load()
        rc = lib.sslrec_au_bwd_f32(n, n_user, d, ia.data_ptr(), ip.data_ptr(), B, scale, gamma, terms, out.data_ptr(), ga.data_ptr(),
                                   gu.data_ptr(), grad.data_ptr(), ctx.ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_au_bwd_f32')
        return grad, None, None, None, None, None, None


def _au_fused(table, n_user, ancs, poss, gamma, scale, terms):
    d = table.shape[1]
    return _AlignUniformFn.apply(_pad_cols(table, _padded_dim(d, AU_DIMS)), n_user, ancs, poss, gamma, scale, terms)


def align_uniform_loss_stacked(table, n_user, ancs, poss, gamma, scale=1.0):
    """(loss, align_loss, uniform_loss) of DirectAU (directau.py:43-47, loss_utils.py:75-86) on the stacked table [users; items] [N, d]:
    with x = normalize(scale * table[ancs]) and y = normalize(scale * table[n_user + poss]),
        align_loss = mean |x - y|^2,  uniform_loss = gamma * (uniformity(x) + uniformity(y)) / 2,  loss = their sum
    as ONE autograd node returning three 0-d tensors; the gradient reaches `table` only.  `scale` folds the mean over the layers
    (directau.py:35) into the gather: pass the layer SUM of ops.propagate_sum and scale = 1 / (L + 1).  No [B, B] or [B (B - 1) / 2]
    tensor forward or backward; duplicated indices are ordinary pairs (a pair is left out by batch position only); two runs give the
    same bits.  Embedding sizes without a kernel are zero-padded.  What the kernels do not cover runs the reference's torch
    expression: B < 2 or an empty table (NaN, as the mean of an empty pdist is), B > 8192, d > 128."""
    _need_gpu(table, ancs, poss)
    n_user, gamma, scale = int(n_user), float(gamma), float(scale)
    if table.dim() != 2 or ancs.dim() != 1 or poss.dim() != 1 or tuple(ancs.shape) != tuple(poss.shape) or not 0 <= n_user <= table.shape[0]:
        raise ValueError('align_uniform_loss_stacked: table %s, n_user %d, ancs %s, poss %s ([N, d], 0 <= n_user <= N, two [B] index vectors)'
                         % (tuple(table.shape), n_user, tuple(ancs.shape), tuple(poss.shape)))
    if gamma != gamma or scale != scale or abs(gamma) == float('inf') or abs(scale) == float('inf'):
        raise ValueError('align_uniform_loss_stacked: gamma and scale must be finite, got %r and %r' % (gamma, scale))
    B = int(ancs.shape[0])
    if B < 2 or B > AU_MAX_BATCH or table.shape[0] == 0 or table.shape[1] == 0 or table.shape[1] > AU_DIMS[-1]:
        return _au_composed(table, n_user, ancs.long(), poss.long(), gamma, scale)
    return _au_fused(table, n_user, ancs, poss, gamma, scale, AU_ALIGN | AU_UNIFORM_ANC | AU_UNIFORM_POS)


def _au_dense_ok(x):
    return 2 <= x.shape[0] <= AU_MAX_BATCH and 1 <= x.shape[1] <= AU_DIMS[-1]


def alignment(x, y, alpha=2):
    """loss_utils.alignment (loss_utils.py:75-79) for dense [B, d] rows on the device: the fused kernels with identity indices over
    [x; y]; alpha != 2 and shapes without a kernel run the reference's expression"""
    _need_gpu(x, y)
    if x.dim() != 2 or tuple(x.shape) != tuple(y.shape):
        raise ValueError('alignment: two [B, d] tensors of one shape expected, got %s and %s' % (tuple(x.shape), tuple(y.shape)))
    if alpha != 2 or not _au_dense_ok(x):
        return _au_alignment(x, y, alpha)
    idx = torch.arange(x.shape[0], device=x.device)
    return _au_fused(torch.cat([x, y], dim=0), x.shape[0], idx, idx, 0.0, 1.0, AU_ALIGN)[1]


def uniformity(x):
    """loss_utils.uniformity (loss_utils.py:82-86) for dense [B, d] rows on the device: the fused kernels with identity indices"""
    _need_gpu(x)
    if x.dim() != 2:
        raise ValueError('uniformity: a [B, d] tensor expected, got %s' % (tuple(x.shape),))
    if not _au_dense_ok(x):
        return _au_uniformity(x)
    idx = torch.arange(x.shape[0], device=x.device)
    return _au_fused(x, 0, idx, idx, 2.0, 1.0, AU_UNIFORM_POS)[2]          # gamma * (0 + uniformity(x)) / 2 with gamma = 2


# ----------------------------------------------------------------------------------------------
# Lloyd's k-means of NCL (KMeansClustering.forward, aug_utils.py:147-157) without the [N, K, d] tensor (csrc/kmeans.hip)
# ----------------------------------------------------------------------------------------------
KMEANS_DIMS = (32, 64, 128)
KMEANS_CENT_BYTES = 64 * 1024          # the centroids sit in LDS
KMEANS_FUSED = os.environ.get('SSLREC_KMEANS_FUSED', '1') != '0'      # 0: the composed torch expression at every size (measurement)
KMEANS_POLL = 8                        # iterations between two looks of the host at the changed-row counters (early exit)
KMEANS_CHUNK_ELEMS = 1 << 22           # composed path: rows per chunk = this / (K d)


def kmeans_fused_ok(K, d):
    """shapes the kernels take: d in KMEANS_DIMS, K * d * 4 <= 64 KiB"""
    return int(d) in KMEANS_DIMS and int(K) >= 1 and int(K) * int(d) * 4 <= KMEANS_CENT_BYTES


def _kmeans_composed(x, cent, max_iter, early_exit, poll):
    """the reference's iteration in torch, over row chunks (never the whole [N, K, d]); the lowest index among equal distances, and
    sums by reductions only (no index_add_, whose float atomics depend on the order of arrival): two runs give the same bits"""
    N, d = x.shape
    K = cent.shape[0]
    rows = max(1, KMEANS_CHUNK_ELEMS // (K * d))
    ks = torch.arange(K, device=x.device)
    prev, pending, it = None, [], 0
    idx = counts = None
    while it < max_iter:
        idx = torch.empty(N, dtype=torch.int64, device=x.device)
        sums = torch.zeros_like(cent)
        for lo in range(0, N, rows):
            xc = x[lo:lo + rows]
            dist = (xc[:, None, :] - cent[None, :, :]).square().sum(-1)
            lowest = dist.min(dim=1, keepdim=True).values
            ic = torch.where(dist == lowest, ks, K).min(dim=1).values
            ic = torch.where(ic == K, 0, ic)                     # (a row of NaN distances: cluster 0, like the kernel)
            idx[lo:lo + rows] = ic
            sums += ((ic[None, :] == ks[:, None]).to(x.dtype)[:, :, None] * xc[None, :, :]).sum(1)
        counts = torch.bincount(idx, minlength=K)                # (integer atomics: exact)
        cent = sums / (counts.to(x.dtype)[:, None] + 1e-6)
        if early_exit:                                           # rows that changed cluster; iteration 0 counts every row
            pending.append((idx != prev).sum() if prev is not None else torch.full((), N, dtype=torch.int64, device=x.device))
        prev = idx
        it += 1
        if early_exit and it < max_iter and len(pending) == poll:
            settled = bool((torch.stack(pending) == 0).any().item())
            pending = []
            if settled:
                break
    return cent, idx, counts.to(x.dtype).reshape(K, 1), it


def kmeans(embeds, centroids0, max_iter=1000, early_exit=True, poll=None):
    """The loop of KMeansClustering.forward (aug_utils.py:149-156) from the initial centroids `centroids0` [K, d] (:147) on
    `embeds` [N, d]: returns (centroids [K, d], idx [N] int64, counts [K, 1], iters_run).  Not differentiable (ncl.py:27-28 calls it
    on .detach()).  Distances in the difference form in fp32, the lowest index among equal distances, deterministic sums; an empty
    cluster has centroid 0 and count 0.  early_exit: the host looks every `poll` iterations (default KMEANS_POLL) at how many rows
    changed cluster and stops once an iteration changed none -- the result is bit for bit that of max_iter iterations;
    iters_run = iterations actually run.  Shapes outside kmeans_fused_ok (and SSLREC_KMEANS_FUSED=0) run the composed expression over
    row chunks."""
    _need_gpu(embeds, centroids0)
    if embeds.dim() != 2 or centroids0.dim() != 2 or embeds.shape[1] != centroids0.shape[1] or embeds.shape[0] < 1 or centroids0.shape[0] < 1:
        raise ValueError('kmeans: embeds [N, d] and centroids0 [K, d] with N, K >= 1 expected, got %s and %s'
                         % (tuple(embeds.shape), tuple(centroids0.shape)))
    max_iter, poll = int(max_iter), int(KMEANS_POLL if poll is None else poll)
    if max_iter < 1 or not 1 <= poll <= 64:
        raise ValueError('kmeans: max_iter >= 1 and 1 <= poll <= 64 expected, got %d and %d' % (max_iter, poll))
    with torch.no_grad():
        x, cent = _f32c(embeds.detach()), _f32c(centroids0.detach())
        (N, d), K = x.shape, cent.shape[0]
        if not (KMEANS_FUSED and kmeans_fused_ok(K, d)) or N > 0x7fffffff:
            return _kmeans_composed(x, cent, max_iter, bool(early_exit), poll)
        if x.data_ptr() % 16:
            x = x.clone()
        cent = cent.clone()                                      # the kernels work in place
        lib = _lib.load()
        ws = torch.empty(lib.sslrec_kmeans_ws_bytes(N, K, d) // 4 + 1, dtype=torch.float32, device=x.device)
        idx = torch.empty(N, dtype=torch.int32, device=x.device)
        counts = torch.empty(K, dtype=torch.float32, device=x.device)
        iters = C.c_int32(0)
        rc = lib.sslrec_kmeans_f32(x.data_ptr(), N, d, K, cent.data_ptr(), idx.data_ptr(), counts.data_ptr(), max_iter, int(bool(early_exit)),
                                   poll, C.byref(iters), ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_kmeans_f32')
        return cent, idx.long(), counts.reshape(K, 1), int(iters.value)


# ----------------------------------------------------------------------------------------------
# GFormer (gformer.py): hop counts from the anchors by a bit-parallel multi-source BFS (csrc/bfs.hip), the PNN layer's position
# features without its [N, A, d] tensors (csrc/pnn.hip), and the per-entry attention of LocalGraph (csrc/gt.hip)
# ----------------------------------------------------------------------------------------------
ANCHOR_MAX = 256                       # anchors the kernels take (four 64-bit words per node)
ANCHOR_MAX_LEVEL = 32766               # levels after which a search that still changes something is an error (int16 hops)
ANCHOR_HOPS_POLL = 8                   # levels between two looks of the host at the per-level counters
ANCHOR_HOPS_FUSED = os.environ.get('SSLREC_ANCHOR_HOPS_FUSED', '1') != '0'      # 0: the composed torch loop at every size (measurement)
PNN_DIMS = (32, 64, 128)
PNN_LDS_BYTES = 128 * 1024
PNN_FUSED = os.environ.get('SSLREC_PNN_FUSED', '1') != '0'                      # 0: the composed torch expression at every size
EDGE_SCORES_FUSED = os.environ.get('SSLREC_EDGE_SCORES_FUSED', '1') != '0'


def _pattern_csr(adj_or_pattern, what):
    """(rowptr int32 [n + 1], col int32 [E], long_rows int32, n, device, coo) of an EdgePattern, or of the forward plan of a graph /
    torch sparse adjacency (square); coo() -> (rows, cols) int64 in CSR order"""
    if isinstance(adj_or_pattern, EdgePattern):
        p = adj_or_pattern
        return p.rowptr, p.col, p.long_rows, p.n, p.device, p.coo
    graph = _pattern_graph(adj_or_pattern, what)
    plan = _plan_of(graph, 'fwd', what)
    if plan.n_rows != plan.n_cols:
        raise ValueError('%s: a square pattern expected, got %d x %d' % (what, plan.n_rows, plan.n_cols))
    csr = plan.device_csr()
    return csr['rowptr'], csr['col'], csr['long_rows'], plan.n_rows, plan.device, lambda: (csr['row_of_entry'].long(), csr['col'].long())


def _anchor_ids(anchors, n, what, distinct=True):
    """the anchors as a validated CPU int64 tensor: 1-d, inside [0, n), distinct (unless distinct=False)"""
    a = torch.as_tensor(np.asarray(anchors.detach().cpu()) if torch.is_tensor(anchors) else np.asarray(anchors)).long().reshape(-1)
    if a.numel() < 1:
        raise ValueError('%s: at least one anchor expected' % what)
    if int(a.min()) < 0 or int(a.max()) >= n:
        raise ValueError('%s: an anchor lies outside [0, %d)' % (what, n))
    if distinct and torch.unique(a).numel() != a.numel():
        raise ValueError('%s: the anchors must be distinct' % what)
    return a


def hop_weights(hops, dtype=torch.float32):
    """the reference's weights from hop counts: float32(1 / (hop + 1)), 0 for an unreached node (gformer.py:172-174, :205), as `dtype`"""
    w = (1.0 / (hops.double() + 1.0)).float()
    return torch.where(hops < 0, torch.zeros((), dtype=torch.float32, device=hops.device), w).to(dtype)


def _anchor_hops_composed(rows, cols, n, anchors, max_level=ANCHOR_MAX_LEVEL):
    """the same level-synchronous search with torch ops, 64 anchors at a time: (hops int16 [n, A], levels that changed something)"""
    dev = rows.device
    A = anchors.numel()
    hops = torch.full((n, A), -1, dtype=torch.int16, device=dev)
    most = 0
    for lo in range(0, A, 64):
        anc = anchors[lo:lo + 64].to(dev)
        ar = torch.arange(anc.numel(), device=dev)
        reached = torch.zeros(n, anc.numel(), dtype=torch.bool, device=dev)
        reached[anc, ar] = True
        h = torch.full((n, anc.numel()), -1, dtype=torch.int16, device=dev)
        h[anc, ar] = 0
        level = 0
        while True:
            seen = torch.zeros(n, anc.numel(), dtype=torch.int32, device=dev).index_add_(0, rows, reached[cols].to(torch.int32)) > 0
            new = seen & ~reached
            if not bool(new.any()):
                break
            level += 1
            if level >= max_level:
                raise RuntimeError('anchor_hops: the search has not converged after %d levels' % max_level)
            h[new] = level
            reached |= new
        hops[:, lo:lo + 64] = h
        most = max(most, level)
    return hops, most


def anchor_hops_fused_ok(n, A):
    """shapes csrc/bfs.hip takes: 1 <= A <= 256 anchors, 1 <= n < 2^31 nodes"""
    return 1 <= int(A) <= ANCHOR_MAX and 1 <= int(n) < 2 ** 31 - 1


def anchor_hops(adj_or_pattern, anchors, poll=None, return_levels=False):
    """hops int16 [N, A]: the number of edges on a shortest path from anchor a to node n in the pattern of `adj_or_pattern` (a
    graph.EdgePattern, a PropGraph / RevaluedView, or a torch sparse adjacency), 0 for the anchor itself, -1 for a node it does not
    reach -- what gformer.py:152-176 computes with one networkx BFS per anchor; the reference's `dists_array` is the transpose as
    float64 weights 1 / (hop + 1) (ops.hop_weights).  The pattern must be SYMMETRIC, as the reference's nx.Graph makes it; that is
    not checked.  `anchors`: A distinct node ids (ValueError otherwise).  Exact (integers only).  The host looks every `poll` levels
    (default ANCHOR_HOPS_POLL) at how many rows gained an anchor and stops after a level that changed nothing; the result does not
    depend on `poll`.  A search that still changes something after 32766 levels raises.  1 <= A <= 256 runs csrc/bfs.hip; anything
    else (and SSLREC_ANCHOR_HOPS_FUSED=0) runs a composed torch loop with the same result.  return_levels: (hops, levels that changed
    something)."""
    rowptr, col, long_rows, n, dev, coo = _pattern_csr(adj_or_pattern, 'anchor_hops')
    if torch.device(dev).type != 'cuda':
        raise RuntimeError('sslrec_amd kernels run on a HIP device only (got a %s pattern); there is no CPU fallback by design' % (dev,))
    ids = _anchor_ids(anchors, n, 'anchor_hops')
    A = ids.numel()
    poll = int(ANCHOR_HOPS_POLL if poll is None else poll)
    if not 1 <= poll <= 64:
        raise ValueError('anchor_hops: 1 <= poll <= 64 expected, got %d' % poll)
    with torch.no_grad():
        if not (ANCHOR_HOPS_FUSED and anchor_hops_fused_ok(n, A)):
            rows, cols = coo()
            hops, levels = _anchor_hops_composed(rows, cols, n, ids)
            return (hops, levels) if return_levels else hops
        lib = _lib.load()
        anc = ids.to(torch.int32).to(dev)
        hops = torch.empty(n, A, dtype=torch.int16, device=dev)
        ws = torch.empty(lib.sslrec_anchor_hops_ws_bytes(n, A) // 8 + 1, dtype=torch.int64, device=dev)
        levels, converged = C.c_int32(0), C.c_int32(0)
        rc = lib.sslrec_anchor_hops(rowptr.data_ptr(), col.data_ptr() if col.numel() else ws.data_ptr(), n,
                                    long_rows.data_ptr() if long_rows.numel() else None, long_rows.numel(), anc.data_ptr(), A,
                                    hops.data_ptr(), poll, C.byref(levels), C.byref(converged), ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_anchor_hops')
        if not converged.value:
            raise RuntimeError('anchor_hops: the search has not converged after %d levels' % ANCHOR_MAX_LEVEL)
        return (hops, int(levels.value)) if return_levels else hops


def anchor_position_fused_ok(d, A):
    """shapes csrc/pnn.hip takes: d in {32, 64, 128}, 1 <= A <= 256 anchors whose rows fit 128 KiB of LDS"""
    return int(d) in PNN_DIMS and 1 <= int(A) <= ANCHOR_MAX and int(A) * int(d) * 4 <= PNN_LDS_BYTES


def _anchor_position_composed(x, anchor_ids, hops):
    """[s, u] [N, 2d] in torch, any dtype and device: the collapsed form of gformer.py:202-218 with the cyclic window of the
    reference's repeat / reshape -- s = w @ x[anchors] / A, u[n] = sum_a x[(n A + a) mod N] / A as A row gathers, never an [N, A, d]"""
    N, d = x.shape
    A = anchor_ids.numel()
    w = hop_weights(hops, x.dtype)
    s = (w @ x[anchor_ids.long()]) / A
    start = (torch.arange(N, device=x.device, dtype=torch.int64) * A) % N
    u = torch.zeros_like(x)
    for a in range(A):
        u = u + x[(start + a) % N]
    return torch.cat([s, u / A], dim=1)


class _AnchorPositionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchors, hops):
        x = _f32c(x)
        if x.data_ptr() % 16:
            x = x.clone()
        N, d = x.shape
        z = torch.empty(N, 2 * d, dtype=torch.float32, device=x.device)
        rc = _lib.load().sslrec_pnn_fwd_f32(x.data_ptr(), N, d, anchors.data_ptr(), anchors.numel(), hops.data_ptr(), z.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_pnn_fwd_f32')
        ctx.anchors, ctx.hops, ctx.shape = anchors, hops, (N, d)
        return z

    @staticmethod
    def backward(ctx, gz):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        gz = _f32c(gz)
        if gz.data_ptr() % 16:
            gz = gz.clone()
        N, d = ctx.shape
        A = ctx.anchors.numel()
        lib = _lib.load()
        dx = torch.empty(N, d, dtype=torch.float32, device=gz.device)
        ws = torch.empty(lib.sslrec_pnn_bwd_ws_bytes(N, A, d) // 4 + 1, dtype=torch.float32, device=gz.device)
        rc = lib.sslrec_pnn_bwd_f32(gz.data_ptr(), N, d, ctx.anchors.data_ptr(), A, ctx.hops.data_ptr(), dx.data_ptr(), ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_pnn_bwd_f32')
        return dx, None, None


def anchor_position_features(x, anchor_ids, hops):
    """z [N, 2d] = [s, u], the two feature halves of GFormer's PNNLayer (gformer.py:202-218) with its Linear(2d, d) commuted past the
    mean over the anchors -- the model applies F.linear(z, linear_hidden.weight, linear_hidden.bias):
        s[n] = (1 / A) sum_a w[n, a] x[anchor_ids[a]],  w = float32(1 / (hops[n, a] + 1)), 0 where hops[n, a] < 0 (ops.anchor_hops)
        u[n] = (1 / A) sum_{a < A} x[(n A + a) mod N]
    The window in u is what the reference's `embeds.repeat(A, 1).reshape(-1, A, d)` holds at [n, a]: NOT row n.  For A = 1
    the reference's `.squeeze()` drops the anchor axis and `mean(dim=1)` then averages over the features; this op is defined by the
    un-squeezed expression.  `anchor_ids`: A ids in [0, N) (distinct in the model; a repeated id is handled exactly) -- validated when given
    on the host; an int32 DEVICE tensor is trusted (the model validates once per epoch): an id outside [0, N) in it gives an undefined
    RESULT without an error (the kernels never touch memory outside the tables).  `hops`: int16 [N, A].  Differentiable in x; no float atomics, two runs give the
    same bits; nothing of size N x A x d is stored.  d in {32, 64, 128} with A <= 256 and A d 4 <= 128 KiB run csrc/pnn.hip
    (anchor_position_fused_ok); other shapes, and SSLREC_PNN_FUSED=0, run the composed torch expression."""
    _need_gpu(x, hops)
    if x.dim() != 2 or hops.dim() != 2 or hops.shape[0] != x.shape[0] or hops.dtype != torch.int16:
        raise ValueError('anchor_position_features: x [N, d] and hops int16 [N, A] expected, got %s and %s %s'
                         % (tuple(x.shape), hops.dtype, tuple(hops.shape)))
    N, d = x.shape
    if torch.is_tensor(anchor_ids) and anchor_ids.is_cuda and anchor_ids.dtype == torch.int32:
        anc = anchor_ids.reshape(-1).contiguous()
    else:
        anc = _anchor_ids(anchor_ids, N, 'anchor_position_features', distinct=False).to(torch.int32).to(x.device)
    A = anc.numel()
    if hops.shape[1] != A or N < 1:
        raise ValueError('anchor_position_features: %d anchors for hops of shape %s' % (A, tuple(hops.shape)))
    hops = hops.contiguous()
    if not (PNN_FUSED and anchor_position_fused_ok(d, A)) or N >= 2 ** 31 - 1:
        return _anchor_position_composed(x.float(), anc, hops)
    return _AnchorPositionFn.apply(x.float(), anc, hops)


def _edge_attention_scores_composed(pattern, q, k, head_num):
    """att.sum(-1) of gformer.py:235-250 on the node tables, entries in the order of pattern.coo()"""
    n, d = q.shape
    rows, cols = pattern.coo()
    dh = d // head_num
    # (an element-wise product and a sum, not einsum: einsum turns 'ehd, ehd -> eh' into a batched GEMM of E * H batches of 1 x dh x 1)
    att = torch.exp(torch.clamp((q[rows].view(-1, head_num, dh) * k[cols].view(-1, head_num, dh)).sum(-1), -10.0, 10.0))
    norm = torch.zeros(n, head_num, dtype=q.dtype, device=q.device).index_add_(0, rows, att)[rows]
    return (att / (norm + 1e-8)).sum(-1)


def edge_attention_scores(pattern, q, k, head_num):
    """fp32 [E]: per entry (r, c) of `pattern`, in the order of pattern.coo(), sum over the heads of exp(clamp(<q[r, h], k[c, h]>, -10, 10))
    / (row sum of the exponentials + 1e-8) -- `t.sum(atten, dim=-1)` of GFormer's LocalGraph (gformer.py:235-255, :351-352), from the
    projected NODE tables as in ops.edge_attention.  Forward only (the reference detaches it).  The shapes of
    edge_attention_fused_ok run csrc/gt.hip; any other shape runs the composed torch expression."""
    _need_gpu(q, k)
    if not isinstance(pattern, EdgePattern):
        pattern = pattern_of(pattern)
    head_num = int(head_num)
    if q.dim() != 2 or q.shape != k.shape or q.shape[0] != pattern.n:
        raise ValueError('edge_attention_scores: tables %s / %s for a pattern of %d nodes' % (tuple(q.shape), tuple(k.shape), pattern.n))
    d = q.shape[1]
    if head_num < 1 or d % head_num != 0:
        raise ValueError('edge_attention_scores: the embedding size %d is not a multiple of head_num = %d' % (d, head_num))
    with torch.no_grad():
        q, k = _f32c(q.detach().float()), _f32c(k.detach().float())
        if not (EDGE_SCORES_FUSED and edge_attention_fused_ok(d, head_num)):
            return _edge_attention_scores_composed(pattern, q, k, head_num)
        out = torch.empty(pattern.nnz, dtype=torch.float32, device=q.device)
        if pattern.n > 0 and pattern.nnz > 0:
            lib = _lib.load()
            z = torch.empty(lib.sslrec_gt_scores_ws_bytes(pattern.n, d, head_num) // 4 + 1, dtype=torch.float32, device=q.device)
            p = pattern
            rc = lib.sslrec_gt_scores_f32(p.rowptr.data_ptr(), p.col.data_ptr(), p.n, _ptr(p.long_rows) if p.long_rows.numel() else None,
                                          p.long_rows.numel(), q.data_ptr(), k.data_ptr(), d, head_num, out.data_ptr(), z.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_gt_scores_f32')
        return out


# ----------------------------------------------------------------------------------------------
# the stacked parameter table [user_embeds; item_embeds] without the per-forward concatenation (reference lightgcn.py:34)
# ----------------------------------------------------------------------------------------------
def stacked_alias(u, i):
    """the [U + I, d] table whose first U rows ARE `u` and whose last I rows ARE `i`, when the two tensors are adjacent row ranges of one
    contiguous fp32 buffer (how GraphCF allocates its two parameters); None otherwise.  No copy, detached from autograd."""
    if (u.dim() != 2 or i.dim() != 2 or u.shape[1] != i.shape[1] or u.dtype != torch.float32 or i.dtype != torch.float32 or u.device != i.device
            or not u.is_contiguous() or not i.is_contiguous()):
        return None
    if u.data_ptr() + u.numel() * 4 != i.data_ptr():
        return None
    su, si = u.untyped_storage(), i.untyped_storage()
    if su.data_ptr() != si.data_ptr() or (u.storage_offset() + u.numel() + i.numel()) * 4 > su.nbytes():
        return None
    return torch.empty(0, dtype=torch.float32, device=u.device).set_(su, u.storage_offset(), (u.shape[0] + i.shape[0], u.shape[1]), (u.shape[1], 1))


class _StackParamsFn(torch.autograd.Function):
    """cat([u, i]) for two tensors that already lie behind each other in memory: forward is an alias of their buffer, backward hands
    each its row range of the incoming gradient (views: AccumulateGrad keeps them, nothing is copied)"""

    @staticmethod
    def forward(ctx, u, i):
        ctx.n_u = u.shape[0]
        # The alias has a version counter of its own, so autograd cannot see through it that a tensor saved downstream (the table itself:
        # e0 of the regularizer / of the fused steps) changed when a PARAMETER was written in place between forward and backward -- the
        # reference's t.concat made a copy and was immune.  Saving the two parameters here makes autograd check THEIR counters when this
        # node runs backward (every consumer of the alias backpropagates through it): such a write raises instead of giving wrong numbers.
        ctx.save_for_backward(u, i)
        return stacked_alias(u, i)

    @staticmethod
    def backward(ctx, g):
        ctx.saved_tensors          # raises "modified by an inplace operation" when a parameter was written since the forward
        return g[:ctx.n_u], g[ctx.n_u:]


def stack_params(u, i):
    """[u; i] joined to autograd: without a copy when the two are adjacent row ranges of one buffer, else torch.cat"""
    if stacked_alias(u, i) is None:
        return torch.cat([u, i], dim=0)
    return _StackParamsFn.apply(u, i)


# ----------------------------------------------------------------------------------------------
# SimGCL / SGL: the whole training step as ONE autograd node with a hand-written backward
# ----------------------------------------------------------------------------------------------
# SSLREC_ONE_NODE_STEP=0: the models compose the step from the separate autograd nodes above (rounds 1-4; same kernels, plus the stock
# elementwise launches autograd needs between them: table-sized gradient additions, zero fills, scalar arithmetic)
ONE_NODE_STEP = os.environ.get('SSLREC_ONE_NODE_STEP', '1') != '0'


def _backward_chain(adj, G, L, d, axpy=None, sparse=None, sum_in_last=None):
    """g_L = G, g_{l-1} = G + A^T g_l; returns g_0 (the backward pass of the layer-summed propagation over `adj`).  axpy: fused into
    the last product (the regularizer's gradient); sparse: RowBits of G's non-zero rows (first product); sum_in_last: tables added by
    the last product's flush (other chains' results), or None"""
    rsc = _chain_scale(adj, d, L)
    g = G
    for l in range(L):
        last = l == L - 1
        nxt = torch.empty_like(G)
        spmm_raw(adj, g, 'bwd', acc_in=G, acc_out=nxt, want_y=False, axpy=axpy if last else None, x_row_bits=sparse if l == 0 else None,
                 sum_in=sum_in_last if last else None, row_scale=rsc,
                 scale_flags=0 if rsc is None else ((SCALE_PATTERN if l > 0 else 0) | (0 if last else SCALE_ACC)))
        g = nxt
    return g


class _ContrastiveStepFn(torch.autograd.Function):
    """loss = bpr(view3) / B + reg_weight |E0|^2 + cl_weight / B * (infonce(view1_u[a], view2_u[a], view2_u) + infonce(view1_i[p], view2_i[p],
    view2_i)) of SimGCL (simgcl.py:39-55: views = two perturbed propagations + a clean one over ONE adjacency) and SGL (sgl.py:45-65: two
    edge-dropped adjacencies + the clean one) as ONE autograd node on the two parameter tables.  Forward: the fused kernels of the
    separate nodes, no graph in between; the four scalars come out of one launch (sslrec_weighted_sum4_f32).  Backward, by hand:
      * SimGCL: all three views share the backward map (the perturbation's derivative is the identity), so the InfoNCE `all` gradients,
        the scattered anchor rows and the BPR rows are written into ONE table G -- no zero fill, no table addition -- and one chain of L
        products (the regularizer's gradient in the last flush) gives dE0;
      * SGL: three chains over three adjacencies; the two sparse upstream tables (anchor rows, BPR rows) tell their first product which
        rows are non-zero; the last product of the third chain adds the other two results in its flush (or one sslrec_add_tables launch
        where the layout's build has no room for that).
    Returns (loss, bpr, cl_weight * cl / B, reg) -- only `loss` carries gradient."""

    @staticmethod
    def forward(ctx, user_embeds, item_embeds, spec):
        _need_gpu(user_embeds, item_embeds)
        lib = _lib.load()
        e0 = stacked_alias(user_embeds, item_embeds)          # (GraphCF's two parameters share one buffer: no concatenation)
        if e0 is None:
            e0 = torch.cat([_f32c(user_embeds), _f32c(item_embeds)])
        n_user, (N, d), L = int(user_embeds.shape[0]), e0.shape, int(spec['layer_num'])
        dev = e0.device
        if spec['kind'] == 'simgcl':
            v1, v2, v3 = propagate_sum_views(spec['adj'], e0, L, [spec['noises'][0], spec['noises'][1], None], spec['eps'])
            adjs = (spec['adj'],) * 3
        else:
            adjs = tuple(spec['adjs'])
            v1, v2, v3 = (propagate_sum(a, e0, L) for a in adjs)
        ancs, poss, negs, items_cl = (_idx(spec[k]) for k in ('ancs', 'poss', 'negs', 'items_cl'))
        B = int(ancs.numel())
        # BPR on the clean view (lightgcn.py:49-52), already divided by B
        parts = torch.empty(4, dtype=torch.float32, device=dev)      # bpr, infonce users, infonce items, reg
        p3 = v3.data_ptr()
        p3i = p3 + n_user * d * 4
        ws_b = _ticket_ws(dev, lib.sslrec_bpr_ws_bytes(B), 'bpr')
        _lib.check(lib.sslrec_bpr_fwd_f32(p3, ancs.data_ptr(), p3i, poss.data_ptr(), p3i, negs.data_ptr(), B, d, 0, float(B), ws_b.data_ptr(),
                                          parts.data_ptr(), _stream()), 'sslrec_bpr_fwd_f32')
        variant = _variant_code(0, spec.get('precision')) | (INFONCE_FWD_W_BIT if INFONCE_FWD_W else 0)
        sides = [(0, n_user, ancs), (n_user, N - n_user, items_cl)]
        wss = []
        for k, (row0, M, idx) in enumerate(sides):
            Bk, off = int(idx.numel()), row0 * d * 4
            ws = torch.empty(lib.sslrec_infonce_ws_bytes(Bk, M, d) // 4, dtype=torch.float32, device=dev)
            ev = _infonce_event()
            _lib.check(lib.sslrec_infonce_fwd_f32(v1.data_ptr() + off, idx.data_ptr(), v2.data_ptr() + off, idx.data_ptr(), Bk, v2.data_ptr() + off,
                                                  M, d, float(spec['temp']), variant, ws.data_ptr(), parts.data_ptr() + 4 * (1 + k), _stream()),
                       'sslrec_infonce_fwd_f32')
            _infonce_record(ev, 'fwd', Bk, M, d, variant)
            wss.append(ws)
        ws_r = _ticket_ws(dev, lib.sslrec_sumsq_ws_bytes(), 'sumsq')
        _lib.check(lib.sslrec_sumsq_fwd_f32(e0.data_ptr(), e0.numel(), float(spec['reg_weight']), ws_r.data_ptr(), parts.data_ptr() + 12, _stream()),
                   'sslrec_sumsq_fwd_f32')
        out = torch.empty(6, dtype=torch.float32, device=dev)
        w_cl = float(spec['cl_weight']) / B
        pp = parts.data_ptr()
        _lib.check(lib.sslrec_weighted_sum4_f32(pp, 1.0, pp + 4, w_cl, pp + 8, w_cl, pp + 12, 1.0, out.data_ptr(), _stream()), 'sslrec_weighted_sum4_f32')
        # (the two parameters ride along so that an in-place write to them between forward and backward is detected: e0 may be an alias
        # of their buffer with a version counter of its own, see _StackParamsFn)
        ctx.save_for_backward(e0, v1, v2, v3, ancs, poss, negs, items_cl, *wss, user_embeds, item_embeds)
        ctx.meta = (spec['kind'], adjs, L, n_user, float(spec['temp']), variant, w_cl, float(spec['reg_weight']))
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[5], out[4]

    @staticmethod
    def backward(ctx, g_loss, g_bpr, g_cl, g_reg):
        e0, v1, v2, v3, ancs, poss, negs, items_cl, ws_u, ws_i, _, _ = ctx.saved_tensors
        kind, adjs, L, n_user, temp, variant, w_cl, reg_weight = ctx.meta
        if g_loss is None:
            return None, None, None
        if g_bpr is not None or g_cl is not None or g_reg is not None:
            raise RuntimeError('only the total loss of the fused contrastive step is differentiable (its parts are returned for logging)')
        lib = _lib.load()
        N, d = e0.shape
        dev = e0.device
        B = int(ancs.numel())
        g = g_loss.reshape(1).to(torch.float32).contiguous()
        cs = torch.empty(2, dtype=torch.float32, device=dev)          # (g * cl_weight / B, g)
        _lib.check(lib.sslrec_scalar_scale2_f32(g.data_ptr(), w_cl, 1.0, cs.data_ptr(), _stream()), 'sslrec_scalar_scale2_f32')
        c_cl, c_one = cs.data_ptr(), cs.data_ptr() + 4
        simgcl = kind == 'simgcl'
        # upstream tables of the three views: SimGCL -> one buffer for all of them
        G2 = torch.empty_like(e0)                       # every row is written: `all` operand of one of the two terms
        G1 = G2 if simgcl else torch.zeros_like(e0)     # anchor rows of view 1
        for row0, M, idx, ws in ((0, n_user, ancs, ws_u), (n_user, N - n_user, items_cl, ws_i)):
            Bk, off = int(idx.numel()), row0 * d * 4
            de = torch.empty((2 * Bk, d), dtype=torch.float32, device=dev)
            sws = torch.empty(lib.sslrec_scatter_ws_bytes(2 * Bk) // 4 + 1, dtype=torch.float32, device=dev)
            ev = _infonce_event()
            _lib.check(lib.sslrec_infonce_bwd_scatter_f32(v1.data_ptr() + off, idx.data_ptr(), v2.data_ptr() + off, idx.data_ptr(), Bk,
                                                          v2.data_ptr() + off, M, d, temp, variant, ws.data_ptr(), c_cl, de.data_ptr(),
                                                          G1.data_ptr() + off, G2.data_ptr() + off, G2.data_ptr() + off, sws.data_ptr(), _stream()),
                       'sslrec_infonce_bwd_scatter_f32')
            _infonce_record(ev, 'bwd', Bk, M, d, variant)
        # BPR rows of the clean view: added into the common table (SimGCL), or into a table of their own that the staging launch zeroes (SGL)
        wsb, kept = _bpr_bwd_ws(dev, B, d)
        fused_zero = (not simgcl) and kept and N * d % 4 == 0
        G3 = G2 if simgcl else (torch.empty_like(e0) if fused_zero else torch.zeros_like(e0))
        p3, q3 = v3.data_ptr(), G3.data_ptr()
        p3i, q3i = p3 + n_user * d * 4, q3 + n_user * d * 4
        args = (p3, ancs.data_ptr(), p3i, poss.data_ptr(), p3i, negs.data_ptr(), B, d, 0, float(B), c_one, q3, q3i, q3i, wsb.data_ptr())
        if kept:
            rc = lib.sslrec_bpr_bwd_kept_f32(*args, q3 if fused_zero else None, G3.numel() if fused_zero else 0, _stream())
        else:
            rc = lib.sslrec_bpr_bwd_f32(*args, _stream())
        _check_kept(rc, 'sslrec_bpr_bwd_f32', dev, B, d)
        reg_axpy = (e0, 2.0 * reg_weight, g)
        if simgcl:
            grad = _backward_chain(adjs[0], G2, L, d, axpy=reg_axpy)
        else:
            # (both sparse tables hold the rows ancs / n_user + poss / n_user + negs: SGL's item anchors are [poss; negs], sgl.py:58-59)
            rb3 = RowBits.from_indices(N, ancs, 0, poss, n_user, negs, n_user) if SPARSE_GRAD else None
            rb1 = rb3 if int(items_cl.numel()) == 2 * B else None
            o1 = _backward_chain(adjs[0], G1, L, d, sparse=rb1)
            o2 = _backward_chain(adjs[1], G2, L, d)
            graph3 = adjs[2].graph if isinstance(adjs[2], (DroppedView, RevaluedView)) else adjs[2]
            lay3 = graph3.bwd.swept(d) if graph3.bwd is not None else None
            fold = L >= 1 and lay3 is not None and bool(lib.sslrec_swept_deferred_sum_ok(C.byref(lay3.c_struct())))
            grad = _backward_chain(adjs[2], G3, L, d, axpy=reg_axpy, sparse=rb3, sum_in_last=[o1, o2] if fold else None)
            if not fold:
                _lib.check(lib.sslrec_add_tables_f32(grad.data_ptr(), o1.data_ptr(), o2.data_ptr(), grad.data_ptr(), grad.numel(), _stream()),
                           'sslrec_add_tables_f32')
        return grad[:n_user], grad[n_user:], None


def contrastive_step_ok(adjs, d, n_rows, batch_sizes):
    """can the SimGCL / SGL step run as one node?  (a kernel width for the InfoNCE, batches inside the scatter table, propagation on the
    column-swept or streamed kernels of a PropGraph with both directions)"""
    if not ONE_NODE_STEP or d not in INFONCE_DIMS or d not in SPMM_DIMS or 2 * max(batch_sizes) > 16384 or 3 * min(batch_sizes) > 16384:
        return False
    for a in adjs:
        g = a.graph if isinstance(a, (DroppedView, RevaluedView)) else a
        if not isinstance(g, PropGraph) or g.bwd is None or isinstance(a, RevaluedView):
            return False
    return True


def contrastive_step(user_embeds, item_embeds, spec):
    """(loss, bpr_loss, cl_loss, reg_loss) of a SimGCL / SGL step -- see _ContrastiveStepFn.  spec: kind 'simgcl' (adj, noises = two lists of L
    noise tables / tokens, eps) or 'sgl' (adjs = the three views' adjacencies); layer_num, ancs, poss, negs, items_cl (item anchors of the
    contrastive term: poss for SimGCL, [poss; negs] for SGL), temp, cl_weight, reg_weight, precision"""
    return _ContrastiveStepFn.apply(user_embeds, item_embeds, spec)


class _InfoNceShardedFn(torch.autograd.Function):
    """InfoNCE whose `all` rows are this rank's shard; `reduce(t)` sums a small tensor over the ranks in
    place (B floats forward, B*d floats backward).  Loss and dE1/dE2 come out identical on every rank."""

    @staticmethod
    def forward(ctx, e1, e2, all_local, temp, variant, reduce, will_differentiate=True):
        _need_gpu(e1, e2, all_local)
        e1, e2, all_local = _f32c(e1), _f32c(e2), _f32c(all_local)
        B, d = e1.shape
        M = all_local.shape[0]
        if d not in INFONCE_DIMS:
            raise ValueError('embedding size %d not supported by the HIP InfoNCE (supported: %s)' % (d, INFONCE_DIMS))
        if M == 0:
            raise ValueError('a rank holds no rows of the sharded table')
        lib = _lib.load()
        dev = e1.device
        if INFONCE_FWD_W and will_differentiate and any(ctx.needs_input_grad[:3]):
            variant |= INFONCE_FWD_W_BIT
        ws = torch.empty(lib.sslrec_infonce_ws_bytes(B, M, d) // 4, dtype=torch.float32, device=dev)
        z = torch.empty(B, dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ev = _infonce_event()
        _lib.check(lib.sslrec_infonce_shard_rowsum_f32(e1.data_ptr(), 0, e2.data_ptr(), 0, B, all_local.data_ptr(), M, d,
                                                       float(temp), variant, ws.data_ptr(), z.data_ptr(), _stream()),
                   'sslrec_infonce_shard_rowsum_f32')
        reduce(z)
        _lib.check(lib.sslrec_infonce_shard_loss_f32(B, M, d, variant, ws.data_ptr(), z.data_ptr(), out.data_ptr(),
                                                     _stream()), 'sslrec_infonce_shard_loss_f32')
        _infonce_record(ev, 'fwd', B, M, d, variant)      # (the all-reduce of the B row sums between the two stages included)
        ctx.save_for_backward(ws)
        ctx.meta = (B, M, d, float(temp), variant, reduce)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        (ws,) = ctx.saved_tensors
        B, M, d, temp, variant, reduce = ctx.meta
        g = g.reshape(1).to(torch.float32).contiguous()
        dev = ws.device
        w = torch.empty((B, d), dtype=torch.float32, device=dev)
        dall = torch.empty((M, d), dtype=torch.float32, device=dev)
        de1 = torch.empty((B, d), dtype=torch.float32, device=dev)
        de2 = torch.empty((B, d), dtype=torch.float32, device=dev)
        lib = _lib.load()
        ev = _infonce_event()
        _lib.check(lib.sslrec_infonce_shard_bwd_f32(B, M, d, temp, variant, ws.data_ptr(), g.data_ptr(), w.data_ptr(),
                                                    dall.data_ptr(), _stream()), 'sslrec_infonce_shard_bwd_f32')
        reduce(w)
        _lib.check(lib.sslrec_infonce_shard_finish_bwd_f32(B, M, d, temp, variant, ws.data_ptr(), g.data_ptr(),
                                                           w.data_ptr(), de1.data_ptr(), de2.data_ptr(), _stream()),
                   'sslrec_infonce_shard_finish_bwd_f32')
        _infonce_record(ev, 'bwd', B, M, d, variant)
        return de1, de2, dall, None, None, None, None


def infonce_loss_sharded(embeds1, embeds2, all_local, temp=1.0, variant=0, reduce=None, precision=None):
    """cal_infonce_loss(embeds1, embeds2, all, temp) (loss_utils.py:30-39) with `all` row-sharded:
    `all_local` = this rank's rows, embeds1/embeds2 = the same [B,d] rows on every rank, `reduce` =
    in-place sum over ranks (default: dist.all_reduce).  Returns the full SUM on every rank; the
    gradient w.r.t. all_local is complete for the local rows, w.r.t. embeds1/embeds2 the full one."""
    if reduce is None:
        import torch.distributed as dist
        reduce = dist.all_reduce
    dp = _padded_dim(embeds1.shape[1], INFONCE_DIMS)
    return _InfoNceShardedFn.apply(_pad_cols(embeds1, dp), _pad_cols(embeds2, dp), _pad_cols(all_local, dp), float(temp),
                                   _variant_code(variant, precision), reduce, torch.is_grad_enabled())


# ----------------------------------------------------------------------------------------------
# rank-q products of LightGCL's SVD view
# ----------------------------------------------------------------------------------------------
def _rankq_reduce(m, transposed, x):
    """sum_n M(.,n) x[n,:] -> [q,d];  m is [q,N] (transposed=False) or [N,q] (transposed=True), row-major"""
    q, n = (m.shape[1], m.shape[0]) if transposed else m.shape
    d = x.shape[1]
    lib = _lib.load()
    ws = torch.empty(lib.sslrec_rankq_ws_bytes(q, d) // 4, dtype=torch.float32, device=x.device)
    out = torch.empty((q, d), dtype=torch.float32, device=x.device)
    sq, sn = (1, q) if transposed else (n, 1)
    _lib.check(lib.sslrec_rankq_reduce_f32(m.data_ptr(), sq, sn, x.data_ptr(), n, d, q, ws.data_ptr(), out.data_ptr(), _stream()),
               'sslrec_rankq_reduce_f32')
    return out


def _rankq_expand(m, transposed, s_):
    """y[n,:] = sum_k M(k,n) s[k,:] -> [N,d];  m is [N,q] (transposed=True) or [q,N] (transposed=False), row-major"""
    q, n = (m.shape[1], m.shape[0]) if transposed else m.shape
    d = s_.shape[1]
    y = torch.empty((n, d), dtype=torch.float32, device=s_.device)
    sq, sn = (1, q) if transposed else (n, 1)
    _lib.check(_lib.load().sslrec_rankq_expand_f32(m.data_ptr(), sq, sn, s_.data_ptr(), n, d, q, y.data_ptr(), _stream()),
               'sslrec_rankq_expand_f32')
    return y


def rankq_reduce(m, transposed, x):
    """public form of the rank-q reduction (sharded LightGCL: partial products of a row shard, sslrec_amd/shard.py)"""
    _need_gpu(x, m)
    return _rankq_reduce(_f32c(m), transposed, _f32c(x))


def rankq_expand(m, transposed, s_):
    _need_gpu(s_, m)
    return _rankq_expand(_f32c(m), transposed, _f32c(s_))


class _LowRankFn(torch.autograd.Function):
    """left[N_out,q] @ (right[q,N_in] @ x[N_in,d]) with constant factors (LightGCL's `u_mul_s @ (vt @ E)`,
    lightgcl.py:83-84): two streaming kernels forward, the same two backward (dx = right^T (left^T dy))."""

    @staticmethod
    def forward(ctx, x, left, right):
        _need_gpu(x, left, right)
        x, left, right = _f32c(x), _f32c(left), _f32c(right)
        if left.shape[1] != right.shape[0] or right.shape[1] != x.shape[0] or left.shape[1] > 16:
            raise ValueError('low-rank factors %s, %s do not fit the operand %s (rank <= 16)' % (tuple(left.shape), tuple(right.shape), tuple(x.shape)))
        ctx.save_for_backward(left, right)
        return _rankq_expand(left, True, _rankq_reduce(right, False, x))

    @staticmethod
    def backward(ctx, gy):
        left, right = ctx.saved_tensors
        return _rankq_expand(right, False, _rankq_reduce(left, True, _f32c(gy))), None, None


def lowrank_apply(left, right, x):
    """left @ (right @ x) for rank-q factors (q <= 16), differentiable w.r.t. x"""
    return _LowRankFn.apply(x, left, right)


# ----------------------------------------------------------------------------------------------
# L2 regularizer term
# ----------------------------------------------------------------------------------------------
class _SumSqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        _need_gpu(x)
        x = _f32c(x)
        lib = _lib.load()
        ws = _ticket_ws(x.device, lib.sslrec_sumsq_ws_bytes(), 'sumsq')
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        _lib.check(lib.sslrec_sumsq_fwd_f32(x.data_ptr(), x.numel(), float(weight), ws.data_ptr(), out.data_ptr(), _stream()),
                   'sslrec_sumsq_fwd_f32')
        ctx.save_for_backward(x)
        ctx.weight = float(weight)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.reshape(1).to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        _lib.check(_lib.load().sslrec_sumsq_bwd_f32(x.data_ptr(), x.numel(), ctx.weight, g.data_ptr(), dx.data_ptr(), _stream()),
                   'sslrec_sumsq_bwd_f32')
        return dx, None


def sum_squares(x, weight=1.0):
    """weight * sum of squares of a parameter tensor (= reg_weight * W.norm(2).square() of reg_params,
    loss_utils.py:20-24, lightgcn.py:53) as one fused reduction, with the gradient 2*g*weight*W as one pass"""
    return _SumSqFn.apply(x, float(weight))


# ----------------------------------------------------------------------------------------------
# MHCN (reference models/social/mhcn.py): self-gating, channel attention with the normalised layer sums, hierarchical
# mutual-information loss.  csrc/mhcn.hip holds the row-wise kernels of the last two; the composed torch expressions below take any
# dtype and device, run where no kernel exists (embedding sizes outside MHCN_DIMS, CPU tensors, float64) and are what the kernels are
# measured against (SSLREC_MHCN_FUSED=0).
# ----------------------------------------------------------------------------------------------
MHCN_DIMS = (32, 64, 128)
MHCN_FUSED = os.environ.get('SSLREC_MHCN_FUSED', '1') != '0'      # 0: the composed torch expressions at every size (measurement)
MHCN_NORM_EPS = 1e-12                                             # F.normalize's clamp of the norm


def mhcn_fused_ok(d):
    """embedding sizes csrc/mhcn.hip has kernels for"""
    return int(d) in MHCN_DIMS


def _mhcn_kernel_path(*tensors):
    x = tensors[0]
    return (MHCN_FUSED and x.is_cuda and x.dim() == 2 and mhcn_fused_ok(x.shape[1]) and 1 <= x.shape[0] < 2 ** 31 - 1
            and all(t.is_cuda and t.dtype == torch.float32 for t in tensors))


def _mhcn_table(t):
    """fp32, contiguous, 16-byte aligned (rows are read as float4)"""
    t = _f32c(t)
    return t.clone() if t.data_ptr() % 16 else t


def _mhcn_ws(N, d, device):
    return torch.empty(_lib.load().sslrec_mhcn_ws_bytes(int(N), int(d)) // 4 + 1, dtype=torch.float32, device=device)


def _self_gate_composed(x, weights, biases):
    return tuple(x * torch.sigmoid(torch.nn.functional.linear(x, w, b)) for w, b in zip(weights, biases))


class _SelfGateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, *wb):
        n_gates = len(wb) // 2
        x = _mhcn_table(x)
        N, d = x.shape
        # one stacked copy of the C small tensors, the weights transposed: C d (d + 1) floats
        wt = torch.stack([w.t() for w in wb[:n_gates]]).to(torch.float32).contiguous()
        b = torch.stack(list(wb[n_gates:])).to(torch.float32).contiguous()
        ys = [torch.empty(N, d, dtype=torch.float32, device=x.device) for _ in range(n_gates)]
        rc = _lib.load().sslrec_mhcn_gate_fwd_f32(x.data_ptr(), N, d, wt.data_ptr(), b.data_ptr(), n_gates,
                                                  *([y.data_ptr() for y in ys] + [None] * (4 - n_gates)), _stream())
        _lib.check(rc, 'sslrec_mhcn_gate_fwd_f32')
        ctx.save_for_backward(x, wt, b)          # (the inputs only: the backward recomputes the logits)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        x, wt, b = ctx.saved_tensors
        n_gates = wt.shape[0]
        N, d = x.shape
        gys = [_mhcn_table(g) for g in gys]
        lib = _lib.load()
        dx = torch.empty_like(x)
        dw = torch.empty(n_gates, d, d, dtype=torch.float32, device=x.device)
        db = torch.empty(n_gates, d, dtype=torch.float32, device=x.device)
        ws = torch.empty(lib.sslrec_mhcn_gate_ws_bytes(N, d, n_gates) // 4 + 1, dtype=torch.float32, device=x.device)
        rc = lib.sslrec_mhcn_gate_bwd_f32(x.data_ptr(), N, d, wt.data_ptr(), b.data_ptr(), n_gates,
                                          *([g.data_ptr() for g in gys] + [None] * (4 - n_gates)), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                          ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_mhcn_gate_bwd_f32')
        return (dx, *dw.unbind(0), *db.unbind(0))


def self_gate(x, weights, biases):
    """(Y_1, ..., Y_C), Y_c = x * sigmoid(x @ W_c^T + b_c): the self-gating units of mhcn.py:34-52 for C <= 4 gates that share one
    x [N, d].  weights / biases: those of C nn.Linear(d, d) (out x in layout).  Differentiable in x, every W_c and every b_c.

    One forward launch reads x and writes the C tables, the products on the exact-fp32 MFMA (csrc/mhcn_gate.hip); the backward recomputes
    the logits, so no [N, d] pre-activation or gate tensor is kept, and sums dW_c and db_c from per-workgroup slabs in a fixed order:
    no float atomics, two calls give the same bits.  fp32 HIP tensors with d in {32, 64, 128} run the kernels (mhcn_fused_ok);
    everything else, and SSLREC_MHCN_FUSED=0, the composed torch expression."""
    weights, biases = tuple(weights), tuple(biases)
    if not 1 <= len(weights) <= 4 or len(weights) != len(biases):
        raise ValueError('self_gate: 1 to 4 gates with one bias each expected, got %d and %d' % (len(weights), len(biases)))
    if x.dim() != 2:
        raise ValueError('self_gate: x [N, d] expected, got %s' % (tuple(x.shape),))
    d = x.shape[1]
    for w, b in zip(weights, biases):
        if tuple(w.shape) != (d, d) or tuple(b.shape) != (d,):
            raise ValueError('self_gate: weights [d, d] and biases [d] expected for d = %d, got %s and %s' % (d, tuple(w.shape), tuple(b.shape)))
    if _mhcn_kernel_path(x, *weights, *biases):
        return _SelfGateFn.apply(x, *weights, *biases)
    return _self_gate_composed(x, weights, biases)


def _channel_mix_composed(c1, c2, c3, simp, v, sums=None):
    """(mixed, scores, sums_out) in torch: weight_c = <e_c, v>, softmax over the channels, mixed = sum_c s_c e_c + simp / 2"""
    chans = (c1, c2, c3)
    scores = torch.softmax(torch.stack([e @ v for e in chans], dim=1), dim=-1)
    mixed = simp / 2
    for i, e in enumerate(chans):
        mixed = mixed + scores[:, i:i + 1] * e
    outs = None
    if sums is not None:
        outs = tuple(a + torch.nn.functional.normalize(e, p=2, dim=1, eps=MHCN_NORM_EPS) for a, e in zip(sums, (c1, c2, c3, simp)))
    return mixed, scores, outs


class _ChannelMixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c1, c2, c3, simp, v, *sums):
        tabs = [_mhcn_table(x) for x in (c1, c2, c3, simp)]
        v = _mhcn_table(v)
        accs = [_mhcn_table(a) for a in sums]
        N, d = tabs[0].shape
        dev = tabs[0].device
        mixed = torch.empty(N, d, dtype=torch.float32, device=dev)
        scores = torch.empty(N, 3, dtype=torch.float32, device=dev)
        outs = [torch.empty(N, d, dtype=torch.float32, device=dev) for _ in accs]
        rc = _lib.load().sslrec_mhcn_mix_fwd_f32(*[x.data_ptr() for x in tabs], v.data_ptr(), N, d, *([a.data_ptr() for a in accs] or [None] * 4),
                                                 mixed.data_ptr(), scores.data_ptr(), *([o.data_ptr() for o in outs] or [None] * 4), _stream())
        _lib.check(rc, 'sslrec_mhcn_mix_fwd_f32')
        ctx.save_for_backward(*tabs, v, scores)
        ctx.with_sums = bool(accs)
        ctx.mark_non_differentiable(scores)
        return (mixed, scores, *outs)

    @staticmethod
    def backward(ctx, g_mixed, _g_scores, *g_outs):
        *tabs, v, scores = ctx.saved_tensors
        N, d = tabs[0].shape
        dev = tabs[0].device
        g_mixed = _mhcn_table(g_mixed)
        gos = [_mhcn_table(g) for g in g_outs] if ctx.with_sums else []
        ds = [torch.empty(N, d, dtype=torch.float32, device=dev) for _ in range(4)]
        dv = torch.empty(d, dtype=torch.float32, device=dev)
        ws = _mhcn_ws(N, d, dev)
        rc = _lib.load().sslrec_mhcn_mix_bwd_f32(*[x.data_ptr() for x in tabs], v.data_ptr(), scores.data_ptr(), N, d, g_mixed.data_ptr(),
                                                 *([g.data_ptr() for g in gos] or [None] * 4), *[x.data_ptr() for x in ds], dv.data_ptr(),
                                                 ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_mhcn_mix_bwd_f32')
        return (*ds, dv, *gos)


def channel_mix(c1, c2, c3, simp, v, sums=None, return_scores=False):
    """mixed [N, d] = sum_c s_c e_c + simp / 2 with s = softmax_c(<e_c, v>) per row: `_channel_attention(c1, c2, c3)[0] + simp / 2` of
    mhcn.py:54-64, :81, :112-113.  v [d] = attn_mat @ attn.T is formed by the caller (the reference's (attn * (e @ attn_mat)).sum(1) with
    the product commuted), so autograd carries dv to both parameters.

    sums = (a1, a2, a3, a4): the same launch also returns (a_k + F.normalize(e_k, p=2, dim=1, eps=1e-12))_k for e = (c1, c2, c3, simp),
    the layer sums of :84-101, so the four raw tables are read once.  The clamp of the norm is a clamp: a zero row gives zeros forward
    and g / 1e-12 backward.  return_scores=True appends the [N, 3] scores the reference's `_channel_attention` returns; through the
    kernels they carry no gradient (the model uses them for nothing).

    Returns mixed | (mixed, sums_out) | (mixed, scores) | (mixed, sums_out, scores).  Differentiable in the four tables, v and the four
    sums; backward is one launch over the rows plus the ordered finish for dv; no float atomics, two calls give the same bits.
    fp32 HIP tensors with d in {32, 64, 128} run csrc/mhcn.hip (mhcn_fused_ok); everything else, and SSLREC_MHCN_FUSED=0, the composed
    torch expression."""
    tabs = (c1, c2, c3, simp)
    if any(x.dim() != 2 or x.shape != c1.shape for x in tabs) or v.dim() != 1 or v.shape[0] != c1.shape[1]:
        raise ValueError('channel_mix: four [N, d] tables and v [d] expected, got %s and %s' % ([tuple(x.shape) for x in tabs], tuple(v.shape)))
    if sums is not None:
        sums = tuple(sums)
        if len(sums) != 4 or any(a.shape != c1.shape for a in sums):
            raise ValueError('channel_mix: sums must be four tables of the shape of the channels')
    if _mhcn_kernel_path(*tabs, v, *(sums or ())):
        res = _ChannelMixFn.apply(*tabs, v, *(sums or ()))
        mixed, scores, outs = res[0], res[1], (tuple(res[2:]) if sums is not None else None)
    else:
        mixed, scores, outs = _channel_mix_composed(*tabs, v, sums)
    ret = (mixed,) + ((outs,) if sums is not None else ()) + ((scores,) if return_scores else ())
    return ret[0] if len(ret) == 1 else ret


def _normalize_add_composed(acc, y):
    return acc + torch.nn.functional.normalize(y, p=2, dim=1, eps=MHCN_NORM_EPS)


class _NormalizeAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acc, y):
        acc, y = _mhcn_table(acc), _mhcn_table(y)
        N, d = y.shape
        out = torch.empty_like(y)
        _lib.check(_lib.load().sslrec_mhcn_normadd_fwd_f32(acc.data_ptr(), y.data_ptr(), N, d, out.data_ptr(), _stream()), 'sslrec_mhcn_normadd_fwd_f32')
        ctx.save_for_backward(y)
        return out

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = _mhcn_table(g)
        dy = None
        if ctx.needs_input_grad[1]:
            dy = torch.empty_like(y)
            _lib.check(_lib.load().sslrec_mhcn_normadd_bwd_f32(y.data_ptr(), g.data_ptr(), y.shape[0], y.shape[1], dy.data_ptr(), _stream()),
                       'sslrec_mhcn_normadd_bwd_f32')
        return g, dy


def normalize_add(acc, y):
    """acc + F.normalize(y, p=2, dim=1, eps=1e-12) for one table (the item side, mhcn.py:95-97) as one launch, forward and backward;
    semantics, shapes and the composed path as channel_mix"""
    if acc.shape != y.shape or y.dim() != 2:
        raise ValueError('normalize_add: two [N, d] tables expected, got %s and %s' % (tuple(acc.shape), tuple(y.shape)))
    if _mhcn_kernel_path(y, acc):
        return _NormalizeAddFn.apply(acc, y)
    return _normalize_add_composed(acc, y)


def log_sigmoid_stable(x):
    """log sigmoid(x) = min(x, 0) - log1p(exp(-|x|)), finite for every finite x"""
    return torch.clamp(x, max=0) - torch.log1p(torch.exp(-x.abs()))


def _hier_ssl_composed(em, edge, perms):
    row_u, col_1, row_1, col_2, row_2 = [p.long() for p in perms]
    pos = (em * edge).sum(1)
    neg1 = (em[row_u] * edge).sum(1)
    neg2 = (edge[row_1][:, col_1] * em).sum(1)
    local_ssl = -(log_sigmoid_stable(pos - neg1) + log_sigmoid_stable(neg1 - neg2)).sum()
    graph = edge.mean(0)
    pos = (edge * graph).sum(1)
    neg1 = (edge[row_2][:, col_2] * graph).sum(1)
    global_ssl = -log_sigmoid_stable(pos - neg1).sum()
    return local_ssl + global_ssl


def _inverse_perm(p):
    inv = torch.empty_like(p)
    inv[p.long()] = torch.arange(p.numel(), dtype=p.dtype, device=p.device)
    return inv


class _HierSslFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, em, edge, *perms):
        em, edge = _mhcn_table(em), _mhcn_table(edge)
        N, d = em.shape
        dev = em.device
        coef = torch.empty(N, 3, dtype=torch.float32, device=dev)
        graph = torch.empty(d, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _mhcn_ws(N, d, dev)
        rc = _lib.load().sslrec_mhcn_ssl_fwd_f32(em.data_ptr(), edge.data_ptr(), *[p.data_ptr() for p in perms], N, d, coef.data_ptr(),
                                                 graph.data_ptr(), loss.data_ptr(), ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_mhcn_ssl_fwd_f32')
        ctx.save_for_backward(em, edge, coef, graph, *perms)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        em, edge, coef, graph, *perms = ctx.saved_tensors
        N, d = em.shape
        dev = em.device
        invs = [_inverse_perm(p) for p in perms]          # once per call: a scatter through p is a gather through its inverse
        g = g.reshape(1).to(torch.float32).contiguous()
        d_em = torch.empty(N, d, dtype=torch.float32, device=dev)
        d_edge = torch.empty(N, d, dtype=torch.float32, device=dev)
        ws = _mhcn_ws(N, d, dev)
        rc = _lib.load().sslrec_mhcn_ssl_bwd_f32(em.data_ptr(), edge.data_ptr(), *[p.data_ptr() for p in perms], *[p.data_ptr() for p in invs],
                                                 coef.data_ptr(), graph.data_ptr(), g.data_ptr(), N, d, d_em.data_ptr(), d_edge.data_ptr(),
                                                 ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_mhcn_ssl_bwd_f32')
        return (d_em, d_edge) + (None,) * len(perms)


def hier_ssl_loss(em, edge, perms):
    """The scalar of `_hierarchical_self_supervision` (mhcn.py:121-143) from em [N, d], edge = H @ em (the caller's SpMM, whose backward is
    the existing one) and the five permutations perms = (row_u, col_1, row_1, col_2, row_2) as index tensors: row_shuffle(x) = x[row_u],
    the row_col_shuffle of neg2 = x[row_1][:, col_1], that of the global term = x[row_2][:, col_2] (t.t(t.t(x)[c])[r] equals x[r][:, c]).

    log sigmoid(x) is computed as min(x, 0) - log1p(exp(-|x|)).  This equals the reference's `sigmoid().log()` wherever that is finite
    and stays finite where the reference returns -inf (arguments below about -104 in float32).  The loss is accumulated in double.
    Differentiable in em and edge; the permutations must be permutations (on the kernel path an index outside its range gives an
    undefined result, never an access outside the tables; a repeated index gives the forward of that index list and a backward that is
    not its gradient).  No [N, d] shuffled copy is made in either direction, no float atomics, two calls give the same bits.  fp32 HIP
    tensors with d in {32, 64, 128} run csrc/mhcn.hip; everything else, and SSLREC_MHCN_FUSED=0, the composed torch expression."""
    perms = tuple(perms)
    if em.dim() != 2 or edge.shape != em.shape or len(perms) != 5:
        raise ValueError('hier_ssl_loss: em and edge [N, d] and five permutations expected')
    N, d = em.shape
    for p, n in zip(perms, (N, d, N, d, N)):
        if p.dim() != 1 or p.numel() != n or p.dtype not in (torch.int32, torch.int64):
            raise ValueError('hier_ssl_loss: the permutations (row_u, col_1, row_1, col_2, row_2) have %d, %d, %d, %d, %d integer entries' % (N, d, N, d, N))
    if _mhcn_kernel_path(em, edge):
        return _HierSslFn.apply(em, edge, *[p.to(device=em.device, dtype=torch.int32).contiguous() for p in perms])
    return _hier_ssl_composed(em, edge, [p.to(em.device) for p in perms])


# ----------------------------------------------------------------------------------------------
# KGIN (reference models/kg/kgin.py): the relational aggregation over a typed knowledge graph and the factor modulation of the user
# side (csrc/kgin.hip).  The composed torch expressions below take any dtype and device, run where no kernel exists (embedding sizes
# outside KGIN_DIMS, CPU tensors, float64) and are what the kernels are measured against (SSLREC_KGIN_FUSED=0).
# ----------------------------------------------------------------------------------------------
KGIN_DIMS = (32, 64, 128)
KGIN_FMAX = 8
KGIN_FUSED = os.environ.get('SSLREC_KGIN_FUSED', '1') != '0'      # 0: the composed torch expressions at every size (measurement)


def kgin_fused_ok(d):
    """embedding sizes csrc/kgin.hip has kernels for"""
    return int(d) in KGIN_DIMS


def _kgin_kernel_path(*tensors):
    x = tensors[0]
    return (KGIN_FUSED and x.is_cuda and x.dim() == 2 and kgin_fused_ok(x.shape[1]) and 1 <= x.shape[0] < 2 ** 31 - 1
            and all(t.is_cuda and t.dtype == torch.float32 for t in tensors))


def _kept_edges(graph, keep):
    h, t, r = graph.head, graph.tail, graph.rel
    if keep is not None:
        sel = keep.to(h.device).bool()
        h, t, r = h[sel], t[sel], r[sel]
    return h, t, r


def _rel_aggregate_composed(graph, x, w, keep=None):
    """scatter_mean as index_add_ divided by the clamped count (there is no torch_scatter): the [E, d] gather and product exist here.
    On a HIP device index_add_ and the backward of the two gathers add with float atomics in an order that changes from call to call;
    there the same expression and its gradient run with torch's deterministic algorithms switched on for the duration of the call
    (_RelAggregateComposedFn), so this form too gives the same bits twice."""
    if x.is_cuda:
        return _RelAggregateComposedFn.apply(x, w, graph, keep)
    h, t, r = _kept_edges(graph, keep)
    msg = x[t] * w[r]
    y = torch.zeros(graph.n, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, h, msg)
    cnt = torch.zeros(graph.n, dtype=x.dtype, device=x.device).index_add_(0, h, torch.ones(h.numel(), dtype=x.dtype, device=x.device))
    return y / cnt.clamp(min=1).unsqueeze(1)


class _DeterministicTorch:
    """torch.use_deterministic_algorithms(True) for a block, the previous setting restored afterwards"""

    def __enter__(self):
        self.was = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
        torch.use_deterministic_algorithms(True)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.was[0], warn_only=self.was[1])


class _RelAggregateComposedFn(torch.autograd.Function):
    """the composed expression and its gradient on a HIP device, every index_add_ in torch's deterministic form"""

    @staticmethod
    def forward(ctx, x, w, graph, keep):
        h, t, r = _kept_edges(graph, keep)
        with _DeterministicTorch():
            y = torch.zeros(graph.n, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, h, x[t] * w[r])
            cnt = torch.zeros(graph.n, dtype=x.dtype, device=x.device).index_add_(0, h, torch.ones(h.numel(), dtype=x.dtype, device=x.device))
        inv = 1 / cnt.clamp(min=1).unsqueeze(1)
        ctx.graph, ctx.keep = graph, keep
        ctx.save_for_backward(x, w, inv)
        return y * inv

    @staticmethod
    def backward(ctx, g):
        x, w, inv = ctx.saved_tensors
        h, t, r = _kept_edges(ctx.graph, ctx.keep)
        ge = (g * inv)[h]
        dx = dw = None
        with _DeterministicTorch():
            if ctx.needs_input_grad[0]:
                dx = torch.zeros_like(x).index_add_(0, t, ge * w[r])
            if ctx.needs_input_grad[1]:
                dw = torch.zeros_like(w).index_add_(0, r, ge * x[t])
        return dx, dw, None, None


class _RelAggregateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, graph, keep):
        x, w = _mhcn_table(x), _mhcn_table(w)
        N, d = x.shape
        dev = x.device
        ls = graph.by_head
        y = torch.empty(N, d, dtype=torch.float32, device=dev)
        cnt = torch.empty(N, dtype=torch.int32, device=dev)
        part = torch.empty(max(ls.n_chunks, 1), d, dtype=torch.float32, device=dev)
        part_cnt = torch.empty(max(ls.n_chunks, 1), dtype=torch.int32, device=dev)
        rc = _lib.load().sslrec_kgin_rel_fwd_f32(*ls.c_args(), x.data_ptr(), w.data_ptr(), w.shape[0], d, _ptr(keep) or None, cnt.data_ptr(),
                                                 y.data_ptr(), part.data_ptr(), part_cnt.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_kgin_rel_fwd_f32')
        ctx.graph, ctx.keep = graph, keep
        ctx.save_for_backward(x, w, cnt)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, cnt = ctx.saved_tensors
        graph, keep = ctx.graph, ctx.keep
        g = _mhcn_table(g)
        N, d = x.shape
        dev = x.device
        lib = _lib.load()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            ls = graph.by_tail
            dx = torch.empty(N, d, dtype=torch.float32, device=dev)
            part = torch.empty(max(ls.n_chunks, 1), d, dtype=torch.float32, device=dev)
            rc = lib.sslrec_kgin_rel_bwd_f32(*ls.c_args(), g.data_ptr(), w.data_ptr(), w.shape[0], 1, d, _ptr(keep) or None, cnt.data_ptr(),
                                             dx.data_ptr(), part.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_kgin_rel_bwd_f32 (dX)')
        if ctx.needs_input_grad[1]:
            ls = graph.by_rel
            dw = torch.empty(w.shape[0], d, dtype=torch.float32, device=dev)
            part = torch.empty(max(ls.n_chunks, 1), d, dtype=torch.float32, device=dev)
            rc = lib.sslrec_kgin_rel_bwd_f32(*ls.c_args(), g.data_ptr(), x.data_ptr(), N, 0, d, _ptr(keep) or None, cnt.data_ptr(),
                                             dw.data_ptr(), part.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_kgin_rel_bwd_f32 (dW)')
        return dx, dw, None, None


def rel_aggregate(graph, x, w, keep=None):
    """Y [N, d] with Y[h] = the mean over the kept edges (h, t, r) of x[t] * w[r], 0 for a head without a kept edge: kgin.py:33-36
    (`scatter_mean(entity_emb[tail] * weight[edge_type - 1], head)`) on a graph.RelGraph whose `rel` is already edge_type - 1.
    x [N, d], w [R, d]; keep: None or one flag per edge (bool / uint8 [E]) in the ORDER THE GRAPH WAS BUILT FROM -- the edge sample of
    `_edge_sampling` as a mask; the kernels read it through the edge ids, so a new sample rebuilds nothing.  Differentiable in x and w.

    One CSR walk each for Y, dX and dW (by head, by tail, by relation): no [E, d] tensor, no float atomics, entries of a row added in the
    graph's edge order, rows and relation lists of more than 512 entries split into 512-entry chunks whose sums are added in chunk order
    by a second launch; two calls give the same bits.  The integer count of kept edges per head is written by the forward and reused by
    the backward.  fp32 HIP tensors with d in {32, 64, 128} run csrc/kgin.hip (kgin_fused_ok); everything else, and SSLREC_KGIN_FUSED=0,
    the composed torch expression (index_add_ and a clamped count, which does form the [E, d] product)."""
    if x.dim() != 2 or w.dim() != 2 or x.shape[0] != graph.n or w.shape[0] != graph.n_rel or w.shape[1] != x.shape[1]:
        raise ValueError('rel_aggregate: x [%d, d] and w [%d, d] expected, got %s and %s' % (graph.n, graph.n_rel, tuple(x.shape), tuple(w.shape)))
    if keep is not None:
        if keep.dim() != 1 or keep.numel() != graph.n_edges or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError('rel_aggregate: keep must hold one bool / uint8 flag per edge (%d)' % graph.n_edges)
    if _kgin_kernel_path(x, w) and graph.by_head is not None and graph.device == x.device:
        if keep is not None:
            keep = keep.to(x.device).to(torch.uint8).contiguous()
        return _RelAggregateFn.apply(x, w, graph, keep)
    return _rel_aggregate_composed(graph, x, w, keep)


def _factor_modulate_composed(agg, u, latent, dmat):
    p = torch.softmax(u @ latent.t(), dim=1)
    return agg * (p @ dmat) + agg


class _FactorModulateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, agg, u, latent, dmat):
        agg, u, latent, dmat = _mhcn_table(agg), _mhcn_table(u), _mhcn_table(latent), _mhcn_table(dmat)
        U, d = agg.shape
        out = torch.empty_like(agg)
        rc = _lib.load().sslrec_kgin_fm_fwd_f32(agg.data_ptr(), u.data_ptr(), latent.data_ptr(), dmat.data_ptr(), U, d, latent.shape[0],
                                                out.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_kgin_fm_fwd_f32')
        ctx.save_for_backward(agg, u, latent, dmat)          # (the inputs only: the backward recomputes the softmax)
        return out

    @staticmethod
    def backward(ctx, g):
        agg, u, latent, dmat = ctx.saved_tensors
        g = _mhcn_table(g)
        U, d = agg.shape
        F_ = latent.shape[0]
        lib = _lib.load()
        d_agg, d_u = torch.empty_like(agg), torch.empty_like(u)
        d_ld = torch.empty(2 * F_, d, dtype=torch.float32, device=agg.device)
        ws = torch.empty(lib.sslrec_kgin_fm_ws_bytes(U, d, F_) // 4 + 1, dtype=torch.float32, device=agg.device)
        rc = lib.sslrec_kgin_fm_bwd_f32(agg.data_ptr(), u.data_ptr(), latent.data_ptr(), dmat.data_ptr(), g.data_ptr(), U, d, F_, d_agg.data_ptr(),
                                        d_u.data_ptr(), d_ld.data_ptr(), ws.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_kgin_fm_bwd_f32')
        return d_agg, d_u, d_ld[:F_], d_ld[F_:]


def factor_modulate(agg, u, latent, dmat):
    """agg * (softmax(u @ latent.T, dim=1) @ dmat) + agg: kgin.py:38-46 with dmat = softmax(disen_weight_att, -1) @ weight [F, d] formed
    by the caller once per forward (so autograd carries its gradient to both parameters).  agg, u [U, d]; latent [F, d].
    Differentiable in all four.

    One launch forward, without the [U, F, d] tensor the reference expands; the backward is one launch over the rows, which recomputes
    the softmax, plus the fixed-order finish of the two [F, d] sums over rows (per-workgroup slabs, no float atomics): two calls give the
    same bits.  fp32 HIP tensors with d in {32, 64, 128} and F <= 8 run csrc/kgin.hip; everything else, and SSLREC_KGIN_FUSED=0, the
    composed torch expression."""
    if agg.dim() != 2 or u.shape != agg.shape or latent.dim() != 2 or latent.shape[1] != agg.shape[1] or dmat.shape != latent.shape:
        raise ValueError('factor_modulate: agg, u [U, d] and latent, dmat [F, d] expected, got %s, %s, %s, %s' %
                         (tuple(agg.shape), tuple(u.shape), tuple(latent.shape), tuple(dmat.shape)))
    if _kgin_kernel_path(agg, u, latent, dmat) and 1 <= latent.shape[0] <= KGIN_FMAX:
        return _FactorModulateFn.apply(agg, u, latent, dmat)
    return _factor_modulate_composed(agg, u, latent, dmat)


# ----------------------------------------------------------------------------------------------
# KGCL (reference models/kg/kgcl.py): the relation-aware graph attention RGAT.agg (:60-72) over a RelGraph (csrc/rgat.hip).  The
# composed torch expression takes any dtype and device, runs where no kernel exists (embedding sizes outside KGIN_DIMS, CPU tensors,
# float64) and is what the kernels are measured against (SSLREC_KGCL_FUSED=0).
# ----------------------------------------------------------------------------------------------
KGCL_FUSED = os.environ.get('SSLREC_KGCL_FUSED', '1') != '0'      # 0: the composed torch expression at every size (measurement)


def _rel_attention_expr(graph, x, p, q, r, keep, slope):
    """the contract of rel_attention in torch: scatter_softmax as exp(s - max of the head) over an index_add_ of the same, scatter_sum as
    index_add_ (there is no torch_scatter); the [E, d] gathers and products exist here.  The per-head maximum is a constant of the
    softmax (a shift changes nothing), so it is taken of the detached logits."""
    h, t, rr = _kept_edges(graph, keep)
    n = graph.n
    s = torch.nn.functional.leaky_relu(((p[h] + q[t]) * r[rr]).sum(-1), slope)
    mx = torch.full((n,), float('-inf'), dtype=s.dtype, device=s.device).scatter_reduce_(0, h, s.detach(), 'amax', include_self=True)
    e = torch.exp(s - mx[h])
    z = torch.zeros(n, dtype=s.dtype, device=s.device).index_add_(0, h, e)
    return torch.zeros(n, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, h, x[t] * (e / z[h]).unsqueeze(1))


class _RelAttentionComposedFn(torch.autograd.Function):
    """the composed expression and its gradient on a HIP device with torch's deterministic algorithms switched on for the duration of both
    (as _RelAggregateComposedFn): the inner graph is built in the forward and differentiated in the backward"""

    @staticmethod
    def forward(ctx, x, p, q, r, graph, keep, slope):
        inner = [a.detach().requires_grad_(need) for a, need in zip((x, p, q, r), ctx.needs_input_grad[:4])]
        with _DeterministicTorch(), torch.enable_grad():
            y = _rel_attention_expr(graph, *inner, keep, slope)
        ctx.inner, ctx.y = inner, y
        return y.detach()

    @staticmethod
    def backward(ctx, g):
        wanted = [a for a in ctx.inner if a.requires_grad]
        with _DeterministicTorch():
            grads = iter(torch.autograd.grad(ctx.y, wanted, g, retain_graph=True))
        return (*[next(grads) if a.requires_grad else None for a in ctx.inner], None, None, None)


def _rel_attention_composed(graph, x, p, q, r, keep=None, slope=0.2):
    if x.is_cuda:
        return _RelAttentionComposedFn.apply(x, p, q, r, graph, keep, slope)
    return _rel_attention_expr(graph, x, p, q, r, keep, slope)


class _RelAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, q, r, graph, keep, slope):
        x, p, q, r = _mhcn_table(x), _mhcn_table(p), _mhcn_table(q), _mhcn_table(r)
        N, d = x.shape
        dev = x.device
        ls = graph.by_head
        y = torch.empty(N, d, dtype=torch.float32, device=dev)
        s = torch.empty(max(graph.n_edges, 1), dtype=torch.float32, device=dev)
        m = torch.empty(N, dtype=torch.float32, device=dev)
        z = torch.empty(N, dtype=torch.float32, device=dev)
        part = torch.empty(max(ls.n_chunks, 1), d, dtype=torch.float32, device=dev)
        part_mz = torch.empty(max(ls.n_chunks, 1), 2, dtype=torch.float32, device=dev)
        rc = _lib.load().sslrec_rgat_fwd_f32(*ls.c_args(), x.data_ptr(), p.data_ptr(), q.data_ptr(), r.data_ptr(), r.shape[0], d, slope,
                                             _ptr(keep) or None, s.data_ptr(), m.data_ptr(), z.data_ptr(), y.data_ptr(), part.data_ptr(),
                                             part_mz.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_rgat_fwd_f32')
        ctx.graph, ctx.keep, ctx.slope = graph, keep, slope
        ctx.save_for_backward(x, p, q, r, y, s, m, z)          # tables, Y and [E]- / [N]-sized vectors: no [E, d] tensor
        return y

    @staticmethod
    def backward(ctx, g):
        x, p, q, r, y, s, m, z = ctx.saved_tensors
        graph, keep, slope = ctx.graph, ctx.keep, ctx.slope
        g = _mhcn_table(g)
        N, d = x.shape
        dev = x.device
        lib = _lib.load()
        kp = _ptr(keep) or None
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        alpha, dl = new(max(graph.n_edges, 1)), new(max(graph.n_edges, 1))
        ls = graph.by_head
        dp, part = new(N, d), new(max(ls.n_chunks, 1), d)
        rc = lib.sslrec_rgat_bwd_head_f32(*ls.c_args(), x.data_ptr(), r.data_ptr(), r.shape[0], d, slope, kp, g.data_ptr(), y.data_ptr(),
                                          s.data_ptr(), m.data_ptr(), z.data_ptr(), alpha.data_ptr(), dl.data_ptr(), dp.data_ptr(),
                                          part.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_rgat_bwd_head_f32')
        dx = dq = dr = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
            ls = graph.by_tail
            dx, dq, part = new(N, d), new(N, d), new(max(ls.n_chunks, 1), 2, d)
            rc = lib.sslrec_rgat_bwd_tail_f32(*ls.c_args(), g.data_ptr(), r.data_ptr(), r.shape[0], d, kp, alpha.data_ptr(), dl.data_ptr(),
                                              dx.data_ptr(), dq.data_ptr(), part.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_rgat_bwd_tail_f32')
        if ctx.needs_input_grad[3]:
            ls = graph.by_rel
            dr, part = new(r.shape[0], d), new(max(ls.n_chunks, 1), d)
            rc = lib.sslrec_rgat_bwd_rel_f32(*ls.c_args(), p.data_ptr(), q.data_ptr(), d, kp, dl.data_ptr(), dr.data_ptr(), part.data_ptr(),
                                             _stream())
            _lib.check(rc, 'sslrec_rgat_bwd_rel_f32')
        return dx, dp, dq, dr, None, None, None


def rel_attention(graph, x, p, q, r, keep=None, slope=0.2):
    """Y [N, d], the edge softmax attention of kgcl.py:60-72 (RGAT.agg) over a graph.RelGraph, with the node tables p = x Wh^T + b and
    q = x Wt^T in place of the per-edge fc(cat(x[head], x[tail])) (ops.rgat_aggregate forms them).  Over the kept edges e = (h, t, rel):

        l_e = <p[h] + q[t], r[rel]>,  s_e = l_e > 0 ? l_e : slope l_e,  a_e = softmax of s over the kept edges of head h,
        Y[h] = sum a_e x[t]    (0 for a head without a kept edge)

    x, p, q [N, d], r [R, d]; keep as in rel_aggregate: None or one bool / uint8 flag per edge in the order the graph was built from, read
    through the edge ids, so a new mask rebuilds nothing.  Differentiable in x, p, q and r.

    fp32 HIP tensors with d in {32, 64, 128} and slope >= 0 run csrc/rgat.hip: one CSR walk by head forward (online softmax; a head of
    more than 512 slots in 512-slot chunks merged in chunk order), and backward one walk each by head (dp, and a_e and dl_e as [E]
    vectors), by tail (dx and dq) and by relation (dr), long lists chunked the same way.  No [E, d] tensor, no float atomics, two calls
    give the same bits.  Everything else, and SSLREC_KGCL_FUSED=0 / ops.KGCL_FUSED = False, runs the composed torch expression
    (index_add_, a per-head amax through scatter_reduce_; on a HIP device under torch's deterministic algorithms)."""
    d = x.shape[1] if x.dim() == 2 else -1
    if x.dim() != 2 or x.shape[0] != graph.n or p.shape != x.shape or q.shape != x.shape or r.dim() != 2 or tuple(r.shape) != (graph.n_rel, d):
        raise ValueError('rel_attention: x, p, q [%d, d] and r [%d, d] expected, got %s, %s, %s and %s' %
                         (graph.n, graph.n_rel, tuple(x.shape), tuple(p.shape), tuple(q.shape), tuple(r.shape)))
    if keep is not None:
        if keep.dim() != 1 or keep.numel() != graph.n_edges or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError('rel_attention: keep must hold one bool / uint8 flag per edge (%d)' % graph.n_edges)
    slope = float(slope)
    if (KGCL_FUSED and slope >= 0 and x.is_cuda and kgin_fused_ok(d) and all(t.is_cuda and t.dtype == torch.float32 for t in (x, p, q, r))
            and graph.by_head is not None and graph.device == x.device):
        if keep is not None:
            keep = keep.to(x.device).to(torch.uint8).contiguous()
        return _RelAttentionFn.apply(x, p, q, r, graph, keep, slope)
    return _rel_attention_composed(graph, x, p, q, r, keep, slope)


def rgat_aggregate(graph, x, fc_weight, fc_bias, rel_emb, keep=None, slope=0.2):
    """RGAT.agg (kgcl.py:60-72) from the module's parameters: fc_weight [d, 2 d] and fc_bias [d] of `fc = Linear(2 d, d)`, rel_emb [R, d]
    the rows the graph's relation ids index.  fc(cat(x[h], x[t])) = x[h] Wh^T + b + x[t] Wt^T with Wh = fc_weight[:, :d] and
    Wt = fc_weight[:, d:], so P = x Wh^T + b and Q = x Wt^T are two [N, d] matmuls and autograd carries dP and dQ to x, fc_weight and
    fc_bias; the rest is rel_attention."""
    d = x.shape[1]
    if tuple(fc_weight.shape) != (d, 2 * d) or tuple(fc_bias.shape) != (d,):
        raise ValueError('rgat_aggregate: fc_weight [%d, %d] and fc_bias [%d] expected, got %s and %s' %
                         (d, 2 * d, d, tuple(fc_weight.shape), tuple(fc_bias.shape)))
    p = torch.addmm(fc_bias, x, fc_weight[:, :d].t())
    q = x @ fc_weight[:, d:].t()
    return rel_attention(graph, x, p, q, rel_emb, keep, slope)


# ----------------------------------------------------------------------------------------------
# KGRec (reference models/kg/kgrec.py): the two-head relational attention AttnHGCN.shared_layer_agg (:63-88) and the rationale scores
# norm_attn_computer (:165-188) over a RelGraph (csrc/rmha.hip).  The composed torch expressions take any dtype and device, run where
# no kernel exists (embedding sizes outside KGIN_DIMS, CPU tensors, float64) and are what the kernels are measured against
# (SSLREC_KGREC_FUSED=0).
# ----------------------------------------------------------------------------------------------
KGREC_FUSED = os.environ.get('SSLREC_KGREC_FUSED', '1') != '0'      # 0: the composed torch expressions at every size (measurement)
KGREC_HEADS = 2


def _mh_logits(graph, t, r, keep):
    """(h, tail, rel, l [E', 2]) of the kept edges: l_ea = sum over head a's columns of t[h] t[tail] r[rel], over sqrt(d / 2)"""
    h, tl, rr = _kept_edges(graph, keep)
    dk = t.shape[1] // KGREC_HEADS
    key = (t[tl] * r[rr]).view(-1, KGREC_HEADS, dk)
    return h, tl, rr, (t[h].view(-1, KGREC_HEADS, dk) * key).sum(-1) / math.sqrt(dk)


def _head_softmax(h, l, n):
    """softmax of the rows of l over the edges of each head entity (scatter_softmax); the per-entity maximum is a constant of the softmax
    and is taken of the detached logits"""
    idx = h if l.dim() == 1 else h.unsqueeze(1).expand(-1, l.shape[1])
    mx = torch.full((n,) + tuple(l.shape[1:]), float('-inf'), dtype=l.dtype, device=l.device).scatter_reduce_(0, idx, l.detach(), 'amax',
                                                                                                             include_self=True)
    e = torch.exp(l - mx[h])
    z = torch.zeros((n,) + tuple(l.shape[1:]), dtype=l.dtype, device=l.device).index_add_(0, h, e)
    return e / z[h]


def _rel_mh_attention_expr(graph, x, t, r, keep):
    """the contract of rel_mh_attention in torch: the [E, d] gathers and products exist here"""
    h, tl, rr, l = _mh_logits(graph, t, r, keep)
    n, d = graph.n, x.shape[1]
    a = _head_softmax(h, l, n)
    val = (x[tl] * r[rr]).view(-1, KGREC_HEADS, d // KGREC_HEADS) * a.unsqueeze(-1)
    return torch.zeros(n, d, dtype=x.dtype, device=x.device).index_add_(0, h, val.reshape(-1, d))


class _RelMhAttentionComposedFn(torch.autograd.Function):
    """the composed expression and its gradient on a HIP device with torch's deterministic algorithms switched on for the duration of both
    (as _RelAttentionComposedFn)"""

    @staticmethod
    def forward(ctx, x, t, r, graph, keep):
        inner = [a.detach().requires_grad_(need) for a, need in zip((x, t, r), ctx.needs_input_grad[:3])]
        with _DeterministicTorch(), torch.enable_grad():
            y = _rel_mh_attention_expr(graph, *inner, keep)
        ctx.inner, ctx.y = inner, y
        return y.detach()

    @staticmethod
    def backward(ctx, g):
        wanted = [a for a in ctx.inner if a.requires_grad]
        with _DeterministicTorch():
            grads = iter(torch.autograd.grad(ctx.y, wanted, g, retain_graph=True))
        return (*[next(grads) if a.requires_grad else None for a in ctx.inner], None, None)


def _rel_mh_attention_composed(graph, x, t, r, keep=None):
    if x.is_cuda:
        return _RelMhAttentionComposedFn.apply(x, t, r, graph, keep)
    return _rel_mh_attention_expr(graph, x, t, r, keep)


class _RelMhAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, r, graph, keep):
        x, t, r = _mhcn_table(x), _mhcn_table(t), _mhcn_table(r)
        N, d = x.shape
        dev = x.device
        ls = graph.by_head
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        y, lg, m, z = new(N, d), new(max(graph.n_edges, 1), 2), new(N, 2), new(N, 2)
        part, part_mz = new(max(ls.n_chunks, 1), d), new(max(ls.n_chunks, 1), 2, 2)
        rc = _lib.load().sslrec_rmha_fwd_f32(*ls.c_args(), x.data_ptr(), t.data_ptr(), r.data_ptr(), r.shape[0], d, _ptr(keep) or None,
                                             lg.data_ptr(), m.data_ptr(), z.data_ptr(), y.data_ptr(), part.data_ptr(), part_mz.data_ptr(),
                                             _stream())
        _lib.check(rc, 'sslrec_rmha_fwd_f32')
        ctx.graph, ctx.keep = graph, keep
        ctx.save_for_backward(x, t, r, y, lg, m, z)            # tables, Y and [E, 2]- / [N, 2]-sized vectors: no [E, d] tensor
        return y

    @staticmethod
    def backward(ctx, g):
        x, t, r, y, lg, m, z = ctx.saved_tensors
        graph, keep = ctx.graph, ctx.keep
        g = _mhcn_table(g)
        N, d = x.shape
        dev = x.device
        lib = _lib.load()
        kp = _ptr(keep) or None
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        alpha, dl = new(max(graph.n_edges, 1), 2), new(max(graph.n_edges, 1), 2)
        ls = graph.by_head
        dt_head, part = new(N, d), new(max(ls.n_chunks, 1), d)
        rc = lib.sslrec_rmha_bwd_head_f32(*ls.c_args(), x.data_ptr(), t.data_ptr(), r.data_ptr(), r.shape[0], d, kp, g.data_ptr(), y.data_ptr(),
                                          lg.data_ptr(), m.data_ptr(), z.data_ptr(), alpha.data_ptr(), dl.data_ptr(), dt_head.data_ptr(),
                                          part.data_ptr(), _stream())
        _lib.check(rc, 'sslrec_rmha_bwd_head_f32')
        dx = dt = dr = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ls = graph.by_tail
            dx, dt_tail, part = new(N, d), new(N, d), new(max(ls.n_chunks, 1), 2, d)
            rc = lib.sslrec_rmha_bwd_tail_f32(*ls.c_args(), g.data_ptr(), t.data_ptr(), r.data_ptr(), r.shape[0], d, kp, alpha.data_ptr(),
                                              dl.data_ptr(), dx.data_ptr(), dt_tail.data_ptr(), part.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_rmha_bwd_tail_f32')
            dt = dt_head.add_(dt_tail)                          # [N, d]: the head's and the tail's share of dT
        if ctx.needs_input_grad[2]:
            ls = graph.by_rel
            dr, part = new(r.shape[0], d), new(max(ls.n_chunks, 1), d)
            rc = lib.sslrec_rmha_bwd_rel_f32(*ls.c_args(), g.data_ptr(), x.data_ptr(), t.data_ptr(), d, kp, alpha.data_ptr(), dl.data_ptr(),
                                             dr.data_ptr(), part.data_ptr(), _stream())
            _lib.check(rc, 'sslrec_rmha_bwd_rel_f32')
        return (dx if ctx.needs_input_grad[0] else None, dt if ctx.needs_input_grad[1] else None, dr, None, None)


def _kgrec_args(name, graph, t, r, keep):
    d = t.shape[1] if t.dim() == 2 else -1
    if t.dim() != 2 or t.shape[0] != graph.n or r.dim() != 2 or tuple(r.shape) != (graph.n_rel, d) or d % KGREC_HEADS:
        raise ValueError('%s: tables [%d, d] with an even d and r [%d, d] expected, got %s and %s' %
                         (name, graph.n, graph.n_rel, tuple(t.shape), tuple(r.shape)))
    if keep is not None:
        if keep.dim() != 1 or keep.numel() != graph.n_edges or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError('%s: keep must hold one bool / uint8 flag per edge (%d)' % (name, graph.n_edges))


def _kgrec_kernel_path(graph, *tensors):
    x = tensors[0]
    return (KGREC_FUSED and x.is_cuda and kgin_fused_ok(x.shape[1]) and all(a.is_cuda and a.dtype == torch.float32 for a in tensors)
            and graph.by_head is not None and graph.device == x.device)


def rel_mh_attention(graph, x, t, r, keep=None):
    """Y [N, d], the two-head attention of kgrec.py:63-82 (AttnHGCN.shared_layer_agg, its entity side) over a graph.RelGraph, with the
    node table t = x W_Q in place of the per-edge `entity_emb[.] @ W_Q` (ops.attn_hgcn_aggregate forms it).  Attention head a owns the
    columns C_a = [a d/2, (a + 1) d/2).  Over the kept edges e = (h, tail, rel):

        l_ea = sum_{C_a} t[h] t[tail] r[rel] / sqrt(d / 2),   al_ea = softmax of l_.a over the kept edges of head entity h,
        Y[h]_j = sum_e al_ea(j) x[tail]_j r[rel]_j    (0 for an entity without a kept edge)

    x, t [N, d], r [R, d]; keep as in rel_aggregate: None or one bool / uint8 flag per edge in the order the graph was built from, read
    through the edge ids, so a new mask rebuilds nothing.  Differentiable in x, t and r.

    fp32 HIP tensors with d in {32, 64, 128} run csrc/rmha.hip: one CSR walk by head forward (online softmax per attention head on the
    two halves of the lane group; an entity of more than 512 slots in 512-slot chunks merged in chunk order), and backward one walk each
    by head (dt's head share, and al and dl as [E, 2] vectors), by tail (dx and dt's tail share) and by relation (dr), long lists chunked
    the same way.  No [E, d] tensor, no float atomics, two calls give the same bits.  Everything else, and SSLREC_KGREC_FUSED=0 /
    ops.KGREC_FUSED = False, runs the composed torch expression (on a HIP device under torch's deterministic algorithms)."""
    if tuple(x.shape) != tuple(t.shape):
        raise ValueError('rel_mh_attention: x and t of one shape expected, got %s and %s' % (tuple(x.shape), tuple(t.shape)))
    _kgrec_args('rel_mh_attention', graph, t, r, keep)
    if _kgrec_kernel_path(graph, x, t, r):
        if keep is not None:
            keep = keep.to(x.device).to(torch.uint8).contiguous()
        return _RelMhAttentionFn.apply(x, t, r, graph, keep)
    return _rel_mh_attention_composed(graph, x, t, r, keep)


def attn_hgcn_aggregate(graph, x, w_q, rel_emb, keep=None):
    """the entity side of AttnHGCN.shared_layer_agg (kgrec.py:63-82) from the module's parameters: w_q [d, d], rel_emb [R, d] the rows the
    graph's relation ids index.  query and key are rows of T = x @ w_q, one [N, d] matmul through which autograd carries dT to x and
    w_q; the rest is rel_mh_attention."""
    d = x.shape[1]
    if tuple(w_q.shape) != (d, d):
        raise ValueError('attn_hgcn_aggregate: w_q [%d, %d] expected, got %s' % (d, d, tuple(w_q.shape)))
    return rel_mh_attention(graph, x, torch.mm(x, w_q), rel_emb, keep)


def _rel_rationale_composed(graph, t, r, keep):
    h, tl, rr, l = _mh_logits(graph, t, r, keep)
    n, E = graph.n, graph.n_edges
    lbar = l.mean(-1)
    ones = torch.ones_like(lbar)
    deg_h = torch.zeros(n, dtype=t.dtype, device=t.device).index_add_(0, h, ones)
    deg_t = torch.zeros(n, dtype=t.dtype, device=t.device).index_add_(0, tl, ones)
    sc = _head_softmax(h, lbar, n) * deg_h[h]
    if keep is None:
        score, logits = sc, lbar
    else:
        sel = keep.to(t.device).bool()
        score = torch.zeros(E, dtype=t.dtype, device=t.device).masked_scatter_(sel, sc)
        logits = torch.zeros(E, dtype=t.dtype, device=t.device).masked_scatter_(sel, lbar)
    mean_head = torch.zeros(n, dtype=t.dtype, device=t.device).index_add_(0, h, sc) / deg_h.clamp(min=1)
    mean_tail = torch.zeros(n, dtype=t.dtype, device=t.device).index_add_(0, tl, sc) / deg_t.clamp(min=1)
    return score, logits, mean_head, mean_tail


@torch.no_grad()
def rel_rationale(graph, t, r, keep=None):
    """(score [E], logits [E], mean_head [N], mean_tail [N]): KGRec's rationale scores, kgrec.py:165-188 (norm_attn_computer) with
    t = entity_emb @ W_Q, and the two scatter_mean calls of :414-417.  Over the kept edges e = (h, tail, rel), with l_ea as in
    rel_mh_attention:

        logits_e = (l_e0 + l_e1) / 2,   score_e = softmax of logits over the kept edges of head entity h, times their number

    both by edge id, 0 for an edge that is not kept; mean_head[n] / mean_tail[n] the mean of score over the kept edges whose head /
    tail is n, 0 where there is none.  No gradient.  fp32 HIP tensors with d in {32, 64, 128} run csrc/rmha.hip (one walk by head for
    the maxima, the sums and the scores, one by tail for the tail mean; no [E, d] tensor, no float atomics, equal bits twice);
    everything else, and ops.KGREC_FUSED = False, the composed torch expression."""
    _kgrec_args('rel_rationale', graph, t, r, keep)
    t, r = t.detach(), r.detach()
    if not _kgrec_kernel_path(graph, t, r):
        if t.is_cuda:
            with _DeterministicTorch():
                return _rel_rationale_composed(graph, t, r, keep)
        return _rel_rationale_composed(graph, t, r, keep)
    if keep is not None:
        keep = keep.to(t.device).to(torch.uint8).contiguous()
    t, r = _mhcn_table(t), _mhcn_table(r)
    N, d = t.shape
    dev = t.device
    E = graph.n_edges
    lib = _lib.load()
    kp = _ptr(keep) or None
    score, logits = torch.zeros(max(E, 1), dtype=torch.float32, device=dev), torch.zeros(max(E, 1), dtype=torch.float32, device=dev)
    mean_head, mean_tail = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
    ls = graph.by_head
    part_mz = torch.empty(max(ls.n_chunks, 1), 2, dtype=torch.float32, device=dev)
    part_cnt = torch.empty(max(ls.n_chunks, 1), dtype=torch.int32, device=dev)
    rc = lib.sslrec_rmha_score_f32(*ls.c_args(), t.data_ptr(), r.data_ptr(), r.shape[0], d, kp, logits.data_ptr(), score.data_ptr(),
                                   mean_head.data_ptr(), part_mz.data_ptr(), part_cnt.data_ptr(), _stream())
    _lib.check(rc, 'sslrec_rmha_score_f32')
    ls = graph.by_tail
    part_sum = torch.empty(max(ls.n_chunks, 1), dtype=torch.float32, device=dev)
    part_cnt = torch.empty(max(ls.n_chunks, 1), dtype=torch.int32, device=dev)
    rc = lib.sslrec_rmha_mean_f32(*ls.c_args(), kp, score.data_ptr(), mean_tail.data_ptr(), part_sum.data_ptr(), part_cnt.data_ptr(), _stream())
    _lib.check(rc, 'sslrec_rmha_mean_f32')
    return score[:E], logits[:E], mean_head, mean_tail


# ----------------------------------------------------------------------------------------------
# all-rank evaluation and negative sampling on the device
# ----------------------------------------------------------------------------------------------
def full_predict(user_table, item_table, users, train_mask=None):
    """[B, I] = (user_table[users] @ item_table.T) * (1 - train_mask) - 1e8 * train_mask: `full_predict` + `_mask_predict` of the
    reference (lightgcn.py:58-66, base_model.py:35-36) in one fused pass -- score tiles on the matrix cores, the mask read once, the
    result written once.  train_mask: [B, I] int64 (the reference's), float32, uint8 or bool, or None."""
    _need_gpu(user_table, item_table)
    ue, ie = _f32c(user_table), _f32c(item_table)
    d = ue.shape[1]
    if d > INFONCE_DIMS[-1]:
        raise ValueError('embedding size %d not supported by the HIP scoring kernel (up to %d)' % (d, INFONCE_DIMS[-1]))
    if d not in INFONCE_DIMS:
        dp = _padded_dim(d, INFONCE_DIMS)
        ue, ie, d = _f32c(_pad_cols(ue, dp)), _f32c(_pad_cols(ie, dp)), dp
    users = _idx(users)
    n_users = int(users.numel()) if users is not None else ue.shape[0]
    n_items = ie.shape[0]
    elem = 0
    if train_mask is not None:
        _need_gpu(train_mask)
        if tuple(train_mask.shape) != (n_users, n_items):
            raise ValueError('train mask of shape %s for %d users x %d items' % (tuple(train_mask.shape), n_users, n_items))
        if train_mask.dtype == torch.bool:
            train_mask = train_mask.view(torch.uint8)
        if train_mask.dtype not in (torch.int64, torch.float32, torch.uint8):
            train_mask = train_mask.to(torch.float32)
        train_mask = train_mask.contiguous()
        elem = train_mask.element_size()
    out = torch.empty((n_users, n_items), dtype=torch.float32, device=ue.device)
    rc = _lib.load().sslrec_full_predict_f32(ue.data_ptr(), _ptr(users), n_users, ie.data_ptr(), n_items, d, _ptr(train_mask), elem,
                                             out.data_ptr(), _stream())
    _lib.check(rc, 'sslrec_full_predict_f32')
    return out


def eval_topk(user_table, item_table, users, k, trn_csr=None, return_scores=False):
    """indices [B, k] (int64) of the k best-scoring items each user has NOT interacted with in training: the fused
    form of full_predict + _mask_predict + t.topk (lightgcn.py:58-66, base_model.py:35-36, metrics.py:99-103).
    `trn_csr` = (rowptr int64 [U+1], col int64 [nnz], sorted inside a row) on the device, or None."""
    _need_gpu(user_table, item_table)
    ue, ie = _f32c(user_table), _f32c(item_table)
    d = ue.shape[1]
    if d > INFONCE_DIMS[-1]:
        raise ValueError('embedding size %d not supported by the HIP evaluation kernel (up to %d)' % (d, INFONCE_DIMS[-1]))
    if int(k) > EVAL_KMAX:
        raise ValueError('k = %d exceeds the HIP evaluation kernel\'s per-user buffers (EVAL_KMAX = %d)' % (int(k), EVAL_KMAX))
    if d not in INFONCE_DIMS:       # other sizes (16 is in the reference's tuning grid): zero columns change no score
        dp = _padded_dim(d, INFONCE_DIMS)
        ue, ie, d = _f32c(_pad_cols(ue, dp)), _f32c(_pad_cols(ie, dp)), dp
    users = _idx(users)
    n_users = int(users.numel()) if users is not None else ue.shape[0]
    n_items = ie.shape[0]
    lib = _lib.load()
    ws = torch.empty(max(lib.sslrec_eval_topk_ws_bytes(n_users, n_items, int(k)), 8) // 4, dtype=torch.float32, device=ue.device)
    out = torch.empty((n_users, int(k)), dtype=torch.int64, device=ue.device)
    val = torch.empty((n_users, int(k)), dtype=torch.float32, device=ue.device) if return_scores else None
    rowptr, col = (None, None) if trn_csr is None else trn_csr
    rc = lib.sslrec_eval_topk_f32(ue.data_ptr(), _ptr(users), n_users, ie.data_ptr(), n_items, d, _ptr(rowptr), _ptr(col), int(k),
                                  ws.data_ptr(), out.data_ptr(), _ptr(val), _stream())
    _lib.check(rc, 'sslrec_eval_topk_f32')
    return (out, val) if return_scores else out


def sample_negs(users, trn_csr, n_item, philox_state, stream_id=None):
    """one negative item per interaction, uniform over the items the user has not interacted with (the distribution of
    datasets_general_cf.py:13-20), drawn on the device from the Philox stream of `philox_state` (sslrec_amd.rng)"""
    users = _idx(users)
    _need_gpu(users)
    rowptr, col = trn_csr
    out = torch.empty_like(users)
    sid = philox_state.next_stream() if stream_id is None else int(stream_id)
    rc = _lib.load().sslrec_sample_negs(users.data_ptr(), users.numel(), rowptr.data_ptr(), col.data_ptr(), int(n_item),
                                        philox_state.state.data_ptr(), sid, out.data_ptr(), _stream())
    _lib.check(rc, 'sslrec_sample_negs')
    return out
