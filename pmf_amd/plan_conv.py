"""Convolution layers of a plan (mixin of pmf_amd.plan.Plan): Conv2d (+bias) -> activation -> BatchNorm forward, and on the
tape the BatchNorm backward, the input gradients (one launch per operand / parity class, or ONE multi-destination launch for
a concatenated input) and the weight gradient (partial slabs + batched reduction on the weight-gradient lanes)."""
import ctypes as C
import os

import torch

from . import _lib as L
from .plan_graph import COL_ROWS, SPLITK_BYTES, _ru, T, V


def _sm(op, p=(), i=(), f=(), l=()):
    """arguments of a small op: pointers, ints, floats and 64-bit ints, each from slot 0 on"""
    a = op.u.sm
    for slots, vals in ((a.p, p), (a.i, i), (a.f, f), (a.l, l)):
        for k, v in enumerate(vals):
            slots[k] = v


def _class_hw(H, W, stride, py, px):
    """the pixels of an H x W map that one input-gradient launch writes: all of them (stride 1) or one parity class"""
    return (H, W) if stride == 1 else ((H - py + 1) // 2, (W - px + 1) // 2)


class PlanConvMixin(object):
    def taps(self, kh, kw, dil, pad):
        out = []
        for ky in range(kh):
            for kx in range(kw):
                out.append((ky * dil - pad, kx * dil - pad, ky * kw + kx))
        return out

    def add_pack(self, weight, taps_widx, transpose, K_pad, ldw, fmt=0, cin=None):
        """register a pack job; returns the Buf of the packed slab [ntaps][K_pad][ldw] (fmt 0, fp32) or of the split-bf16
        fragments [ntaps][K_pad/16][ldw/32][3][64][8] (fmt 1, 6 bytes per weight; pmf_conv_desc_t.w_s3)."""
        # (fmt 2, the stem class: ONE virtual tap, K_pad = taps * 8 rounded up to 16)
        buf = self.persist.alloc((6 if fmt else 4) * (1 if fmt == 2 else len(taps_widx)) * K_pad * ldw)
        # forward packs: index of the conv op about to be emitted (the first reader); input-gradient packs: none (they are
        # read by the backward graph only)
        owner = len(self.fwd) if (not transpose and self.fwd is not None) else None
        # cin = (first input channel, count): pack that channel range only (its own column origin)
        self.pack_jobs.append((weight, buf, list(taps_widx), transpose, K_pad, ldw, self.lane, fmt, owner, cin))
        return buf

    def s3_ok(self, shape_fill):
        """True when this conv launch may run on the bf16 matrix pipe with split operands (conv_fwd.hip PIPE 5)."""
        if not self.s3:
            return False
        probe = L.ConvDesc()
        shape_fill(probe)
        if probe.ntaps == 1:
            # 1x1 layers: only the direct variant (activations straight from global memory, conv_fwd.hip PIPE 11), and only
            # where the map is large enough to fill the chip without a K split
            return (self.s3_direct_min_pix > 0 and probe.N * probe.OH * probe.OW >= self.s3_direct_min_pix
                    and L.lib().pmf_conv_s3_eligible(C.byref(probe)) == 2)
        if probe.ntaps < self.s3_min_taps:
            return False
        return int(L.lib().pmf_conv_s3_eligible(C.byref(probe)))     # (3: the stem class, weights in pack format 2)

    def _live_taps(self, conv, inH, inW, OH, OW):
        """(taps, gather) of a layer.  Taps that can only ever read zero padding (|offset| beyond the map: the dilation-12/18
        ASPP branches on a 4-row map keep 3 of 9 taps) are dropped from forward, input gradient and weight gradient alike;
        their weight gradient is exactly zero and stays at the zero the backward prologue writes."""
        (kh, kw), dil, pad, stride = conv.kernel_size, conv.dilation[0], conv.padding[0], conv.stride[0]
        all_taps = self.taps(kh, kw, dil, pad)
        taps = [(dy, dx, wi) for (dy, dx, wi) in all_taps
                if dy < inH and dy + (OH - 1) * stride >= 0 and dx < inW and dx + (OW - 1) * stride >= 0] or all_taps[:1]
        # very large dilations: per-tap staging (the halo tile would not fit LDS)
        # (rows and columns separately: the dilation-12 / 18 ASPP branches keep one ROW of three taps on the 4-row map -- a
        # 4 x 56-pixel halo tile, not a 32 x 56 one)
        span_y = max(t[0] for t in taps) - min(t[0] for t in taps)
        span_x = max(t[1] for t in taps) - min(t[1] for t in taps)
        return taps, 1 if (8 * stride + span_y) * (32 * stride + span_x) * 80 > 110 * 1024 else 0

    def conv(self, srcs, conv, act=L.ACT_NONE, bn=None, order="act_bn", relu_view=False, name="", pmask=None,
             extra_bias=None):
        """Conv2d (+bias) -> act -> [BatchNorm]  (order 'act_bn', SalsaNext style) or
        Conv2d -> BatchNorm -> [ReLU on the view]  (order 'bn_act', ResNet / attention style).
        Returns a V.  Registers the backward (BN backward, input gradients, weight gradient)."""
        (kh, kw), dil, pad, stride = conv.kernel_size, conv.dilation[0], conv.padding[0], conv.stride[0]
        Cout, N = conv.out_channels, srcs[0].t.N
        inH = max(s.t.H for s in srcs)
        inW = max(s.t.W for s in srcs)
        OH = (inH + 2 * pad - dil * (kh - 1) - 1) // stride + 1
        OW = (inW + 2 * pad - dil * (kw - 1) - 1) // stride + 1
        out = T(self, N, OH, OW, Cout, name)
        taps, gather = self._live_taps(conv, inH, inW, OH, OW)
        # a BatchNorm module in eval mode inside a training plan (frozen statistics, torch semantics): running statistics in
        # the forward pass, no statistics update, backward through the fixed affine map (dgamma / dbeta still flow)
        train_bn = bn is not None and self.training and bn.training
        has_bias = conv.bias is not None
        k_act = act if order == "act_bn" else L.ACT_NONE
        # EPMF SparseVariantConv: (conv + conv.bias + extra bias) * dilated mask; the mask multiplies after the
        # activation (LeakyReLU(0) = 0 and the mask is 0/1, so act(z*m) == act(z)*m) and before the BN statistics
        bsum = None
        if extra_bias is not None:
            if not has_bias:
                raise NotImplementedError("extra_bias needs a conv bias to add to")
            bsum = self.persist.alloc(4 * Cout)
            self.emit(self.fwd, L.OP_VEC_ADD,
                      lambda op: _sm(op, p=(conv.bias.data_ptr(), extra_bias.data_ptr(), bsum.ptr), i=(Cout,)))
        stats, stat_rows = self._conv_forward(srcs, conv, out, taps, gather, k_act, bsum, pmask, train_bn, name)
        view = self._bn_forward(out, bn, train_bn, stats, stat_rows, relu_view) if bn is not None else V(out)
        if name:
            self.views[name] = view
            self.act_sites.append((conv, name, k_act, bool(relu_view)))
        if not self.training:
            return view

        def backward():
            # partial column sums of dz for the conv-bias gradient: one buffer PER LAYER (the weight-gradient op that
            # folds them runs on the side stream while the main stream already works on the next layer)
            dbr = self.act.alloc(COL_ROWS * _ru(Cout, 4) * 4) if (has_bias and pmask is None) else None
            if bn is not None:
                dz, dbias_rows = self._bn_backward(view, k_act, train_bn, dbr, name)
            else:
                dz, dbias_rows = self._act_backward(out, k_act, has_bias, dbr)
            if pmask is not None:
                self._mask_bias_backward(dz, pmask, conv, extra_bias)
            self._dgrad(srcs, conv, dz, taps, stride, gather, name)
            self._wgrad(srcs, conv, dz, taps, stride, gather, name, dbias_rows, dbr, _ru(Cout, 4))
        self.on_backward(backward)
        return view

    def _conv_forward(self, srcs, conv, out, taps, gather, k_act, bsum, pmask, train_bn, name):
        """the forward launch of a layer: kernel class and weight pack, the partial-statistics rows of a training BatchNorm
        behind it, the op.  Returns (statistics rows buffer or None, the row count of the launch as built)."""
        N, OH, OW, Cout, stride = out.N, out.H, out.W, out.C, conv.stride[0]
        Ktot, ldw, has_bias = sum(_ru(s.t.C, 8) for s in srcs), _ru(Cout, 64), conv.bias is not None

        def shape_fill(d):
            d.N, d.OH, d.OW, d.Cout, d.nsrc = N, OH, OW, Cout, len(srcs)
            for i, s in enumerate(srcs):
                d.src[i].C = _ru(s.t.C, 8)
                d.src[i].ldc, d.src[i].H, d.src[i].W = s.t.ldc, s.t.H, s.t.W
                # flags steer the kernel variant (hence the split-K decision the statistics-row probe must match)
                d.src[i].flags = (L.SRC_RELU if s.relu else 0) | (L.SRC_BCAST if s.bcast else 0)
            d.ntaps = len(taps)
            for i, (dy, dx, _) in enumerate(taps):
                d.tdy[i], d.tdx[i] = dy, dx
            d.in_stride, d.gather = stride, gather
            d.out_sy = d.out_sx = 1
            d.splitk_ws, d.splitk_ws_bytes = 1, SPLITK_BYTES      # non-NULL: same split decision as the real launch
            d.splitk_tickets = 1 if self.sk_fused else None          # (... and the same partial-statistics row count)
        fwd_s3 = self.s3_ok(shape_fill)
        if fwd_s3 == 3:
            # the 7x7 RGB stem: 8 padded channels x 49 taps, two taps per 16-deep MFMA step (conv_fwd.hip PIPE 14)
            wbuf = self.add_pack(conv.weight, [t[2] for t in taps], 0, _ru(len(taps) * 8, 16), ldw, 2)
        else:
            wbuf = self.add_pack(conv.weight, [t[2] for t in taps], 0, Ktot, ldw, int(bool(fwd_s3)))
        stat_rows, stats = 0, None
        if train_bn:
            probe = L.ConvDesc()
            shape_fill(probe)
            probe.w_s3 = 1 if fwd_s3 else None
            stat_rows = L.lib().pmf_conv_fwd_stat_rows(C.byref(probe))
            # the autotuner (Plan.autotune) may pick another tile configuration: size the rows for any of them
            max_rows = max(stat_rows, L.lib().pmf_conv_fwd_stat_rows_max(C.byref(probe)))
            stats = self.act.alloc(16 * Cout * max_rows)          # float64 [rows][2][Cout] partials
        lane = self.lane

        def f(op):
            d = op.u.conv
            shape_fill(d)
            for i, s in enumerate(srcs):
                self.src_struct(s, d.src[i])
            d.ldw = ldw
            if fwd_s3:
                d.w_s3 = wbuf.ptr
            else:
                d.w = wbuf.ptr
            d.bias = (bsum.ptr if bsum is not None else conv.bias.data_ptr()) if has_bias else None
            d.act = k_act
            d.out, d.out_ldc, d.out_H, d.out_W = out.buf.ptr, out.ldc, OH, OW
            d.stats = stats.ptr if stats is not None else None
            d.ep_pmask = pmask.buf.ptr if pmask is not None else None
            d.splitk_ws, d.splitk_ws_bytes = self.sk_bufs[lane].ptr, self.sk_bufs[lane].nbytes
            d.splitk_tickets = self.sk_tickets[lane].ptr if self.sk_fused else None
        self.emit(self.fwd, L.OP_CONV, f)
        conv_flops = 2.0 * N * OH * OW * Cout * conv.in_channels * len(taps)   # algorithmic (SURVEY.md 8d rule)
        self.meta_fwd[len(self.fwd) - 1] = dict(family="conv_fwd", flops=conv_flops, name=name, shape="%dx%dx%d %d->%d t%d s%d" % (
            N, OH, OW, conv.in_channels, Cout, len(taps), stride))
        return stats, stat_rows

    def _bn_forward(self, out, bn, train_bn, stats, stat_rows, relu_view):
        """the BatchNorm behind the conv op just emitted: batch statistics from the conv's partial rows (training) or the
        running statistics (eval) -> per-channel scale / shift; returns the view that applies them"""
        Cb = out.C
        scale, shift = self.persist.alloc(4 * Cb), self.persist.alloc(4 * Cb)
        smean, sinv = self.persist.alloc(4 * Cb), self.persist.alloc(4 * Cb)
        if train_bn:
            self.emit(self.fwd, L.OP_BN_FINALIZE, lambda op: _sm(
                op, p=(stats.ptr, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                       bn.running_var.data_ptr(), scale.ptr, shift.ptr, smean.ptr, sinv.ptr),
                f=(float(out.npix), bn.momentum, bn.eps), i=(Cb, stat_rows)))
            self._conv_fin[len(self.fwd) - 2] = len(self.fwd) - 1      # its row count follows the conv's tile config
            self.bn_modules.append(bn)
        else:
            self.emit(self.fwd, L.OP_BN_EVAL, lambda op: _sm(
                op, p=(bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                       scale.ptr, shift.ptr, smean.ptr, sinv.ptr), f=(bn.eps,), i=(Cb,)))
        return V(out, scale, shift, relu=relu_view, bn=dict(mean=smean, invstd=sinv, module=bn))

    # ------------------------------------------------------------------ backward of a layer: dL/d(conv output)
    def _bn_backward(self, view, k_act, train_bn, dbr, name):
        """BatchNorm (+ activation) backward: view.gy, the gradient w.r.t. the BatchNorm output -> out.g, the gradient w.r.t. the
        conv output.  Returns (out.g, number of partial conv-bias-gradient rows written to dbr)."""
        out, bn, mean, invstd = view.t, view.bn["module"], view.bn["mean"], view.bn["invstd"]
        Cout, lane, flag = out.C, self.lane, int(train_bn)
        if getattr(view, "_side", None):
            if view.gy is None:
                view.gy = T(self, out.N, out.H, out.W, Cout, name + ".gy", ldc=out.ldc)
            view.gy_written = self._fold_side(view, view.gy, view.gy_written)
            view._side = None
            view._gy_last = None
        if view.gy is None:
            raise RuntimeError("plan: no gradient reached BN output of %s" % name)
        if out.g is None:
            out.g = T(self, out.N, out.H, out.W, Cout, name + ".dz", ldc=out.ldc)
        out.g_written = True
        coef = self.act.alloc(12 * Cout)                  # [3][Cout] per-channel backward coefficients
        dgam, dbet = self.pgrad(bn.weight), self.pgrad(bn.bias)
        gyt, dz = view.gy, out.g
        self._touch(gyt)
        self._touch(dz)
        self.colrows_max = max(self.colrows_max, _ru(Cout, 4))
        # dgamma and dbeta are complete after the first op emitted below
        self.grad_done[id(bn.weight)] = self.grad_done[id(bn.bias)] = len(self.bwd)
        carry = getattr(view, "_gy_last", None)
        if (os.environ.get("PMF_BN_SMALL", "1") != "0" and Cout % 4 == 0
                and bool(L.lib().pmf_bn_bwd_small_ok(out.npix, Cout))):
            # small maps (<= 2048 pixels: the 4x128 stage and below, a fifth of the BatchNorm layers): column sums,
            # fold and apply in ONE launch (bn.hip bn_bwd_small_k) instead of three latency-bound ones; the
            # input-gradient epilogue then carries no partial sums either (its hook stays empty)
            self.emit(self.bwd, L.OP_BN_BWD_SMALL, lambda op: _sm(
                op, p=(gyt.buf.ptr, out.buf.ptr, mean.ptr, bn.weight.data_ptr(), invstd.ptr, dz.buf.ptr,
                       dbr.ptr if dbr is not None else None, self.pgrad_buf.at(dgam), self.pgrad_buf.at(dbet)),
                i=(gyt.ldc, out.ldc, Cout, flag, k_act, dz.ldc), l=(out.npix,)))
            self.note_bytes(self.bwd, "bn_bwd_small", 12.0 * out.npix * Cout)
            return dz, 1 if dbr is not None else 0
        if carry is not None and carry["lane"] == lane:
            self._bn_bwd_fold(view, carry, coef, dgam, dbet, flag)
        else:
            self.emit(self.bwd, L.OP_BN_BWD_REDUCE, lambda op: _sm(
                op, p=(gyt.buf.ptr, out.buf.ptr, mean.ptr, bn.weight.data_ptr(), invstd.ptr, self.bnpart_bufs[lane].ptr,
                       coef.ptr, self.pgrad_buf.at(dgam), self.pgrad_buf.at(dbet)),
                i=(gyt.ldc, out.ldc, Cout, flag), l=(out.npix,)))
            self.note_bytes(self.bwd, "bn_bwd_reduce", 8.0 * out.npix * Cout)
        self.emit(self.bwd, L.OP_BN_BWD_APPLY, lambda op: _sm(
            op, p=(gyt.buf.ptr, out.buf.ptr, coef.ptr, mean.ptr, dz.buf.ptr, dbr.ptr if dbr is not None else None),
            i=(gyt.ldc, out.ldc, Cout, k_act, dz.ldc, _ru(Cout, 4)), l=(out.npix,)))
        self.note_bytes(self.bwd, "bn_bwd_apply", 12.0 * out.npix * Cout)
        return dz, L.lib().pmf_col_rows(out.npix, Cout) if dbr is not None else 0

    def _arm_bn_carry(self, r, tgt, hook, shape):
        """The BatchNorm carry.  An input-gradient launch that is the LAST writer of the output gradient of a BatchNorm view
        (r.gy) also writes, from its epilogue, the partial column sums that layer's BatchNorm backward needs (sum gy and
        sum gy * (a - mean), one float64 row per output tile); the layer then needs no reduction pass over gy, only the fold.
          * Armed here, by _dgrad_merged and _dgrad_launch, right after they emit a stride-1 launch that writes r.gy itself
            (not a broadcast temporary or another lane's private accumulator): r._gy_last = the launch's still empty hook,
            its op index, its shape filler and its lane.
          * Disarmed by Plan.grad_of: whoever asks for r.gy next is its new last writer (a conv re-arms after its launch, an
            element-wise backward cannot carry the sums); and by _bn_backward when it folds other lanes' accumulators in.
          * Consumed by _bn_bwd_fold when the backward of the layer that produced r is emitted.  It sizes the row buffer with
            the launch's own shape filler -- the row count is the kernel selection's, and a count computed for another kernel
            than the one launched is an out-of-bounds write or uninitialised rows in the sums --, puts the buffer and the
            saved mean into the hook, which _dgrad_epilogue wires into the launch when the plan is finalised, and emits
            OP_BN_BWD_FOLD over the rows.  One-launch BatchNorm backwards (small maps) leave the hook empty.
          * _conv_fold[launch index] lists the fold ops that read a launch's rows (a merged launch feeds one per
            destination): a tile configuration written into the launch later changes its row count, and plan_tune.py
            rewrites the folds' counts through this map.
          * The lane must match: launch and fold hand the rows over in the stream order of one lane, no event in between.
            grad_of gives r.gy itself only to consumers on the producer's lane, so the consumer's test is a guard."""
        if r.bn is not None and tgt is r.gy and self.bn_bwd_fused:
            r._gy_last = dict(hook=hook, index=len(self.bwd) - 1, shape=shape, lane=self.lane)

    def _bn_bwd_fold(self, view, carry, coef, dgam, dbet, flag):
        """consumer of the BatchNorm carry (_arm_bn_carry): the last writer of view.gy was an input-gradient launch on this
        lane that carries the reduction in its epilogue; only the fold of its partial rows is left"""
        out, bn, Cout = view.t, view.bn["module"], view.t.C
        probe = L.ConvDesc()
        carry["shape"](probe)
        nrows = L.lib().pmf_conv_fwd_stat_rows(C.byref(probe))
        rows = self.act.alloc(16 * Cout * max(nrows, L.lib().pmf_conv_fwd_stat_rows_max(C.byref(probe))))
        carry["hook"].update(rows=rows, mean=view.bn["mean"])
        self.emit(self.bwd, L.OP_BN_BWD_FOLD, lambda op: _sm(
            op, p=(rows.ptr, bn.weight.data_ptr(), view.bn["invstd"].ptr, coef.ptr, self.pgrad_buf.at(dgam),
                   self.pgrad_buf.at(dbet)), i=(Cout, nrows, flag), l=(out.npix,)))
        self._conv_fold.setdefault(carry["index"], []).append(len(self.bwd) - 1)

    def _act_backward(self, out, k_act, has_bias, dbr):
        """no BatchNorm: the activation derivative in place on out.g, and the partial rows of the conv-bias gradient"""
        dz, C4 = self.tgrad(out), _ru(out.C, 4)
        if k_act == L.ACT_NONE and not has_bias:
            return dz, 0
        self.emit(self.bwd, L.OP_ACT_BWD, lambda op: _sm(
            op, p=(dz.buf.ptr, out.buf.ptr, dbr.ptr if dbr is not None else None),
            i=(dz.ldc, out.ldc, k_act, C4, C4), l=(out.npix,)))
        self.note_bytes(self.bwd, "act_bwd", 12.0 * out.npix * out.C)
        return dz, L.lib().pmf_col_rows(out.npix, C4) if dbr is not None else 0

    def _mask_bias_backward(self, dz, pmask, conv, extra_bias):
        """d/dz of act(z) * m: the activation derivative was taken from a = act(z)*m (slope of the masked-out zeros is
        irrelevant) -- multiply by the mask, then the bias gradients are plain column sums of the masked dz (both bias
        vectors of SparseVariantConv receive the same gradient)"""
        Cout = dz.C
        self.emit(self.bwd, L.OP_PMASK_MUL_BWD, lambda op: _sm(
            op, p=(dz.buf.ptr, pmask.buf.ptr, dz.buf.ptr), i=(dz.ldc, _ru(Cout, 4), dz.ldc, 0), l=(dz.npix,)))
        if conv.bias is None:
            return
        boff = self.pgrad(conv.bias)
        crows = self.act.alloc(COL_ROWS * _ru(Cout, 4) * 4)      # partial rows of the deterministic column sum
        self.emit(self.bwd, L.OP_COLSUM, lambda op: _sm(
            op, p=(dz.buf.ptr, self.pgrad_buf.at(boff), crows.ptr), i=(dz.ldc, Cout, 1), l=(dz.npix,)))
        self.grad_done[id(conv.bias)] = len(self.bwd) - 1
        if extra_bias is not None:
            eoff = self.pgrad(extra_bias)
            self.emit(self.bwd, L.OP_VEC_ADD, lambda op: _sm(
                op, p=(self.pgrad_buf.at(boff), None, self.pgrad_buf.at(eoff)), i=(Cout,)))
            self.grad_done[id(extra_bias)] = len(self.bwd) - 1

    # ------------------------------------------------------------------ input gradients
    def _dgrad_shape(self, d, dz, Kd, gather, sub, H, W, Cdst, out_stride=None, w_s3=False, dst_C=(), splitk=False):
        """the shape of an input-gradient launch -- what the kernel selection reads -- for probes and launches alike: dz
        (Kd channels) through the taps ``sub`` onto an H x W map of Cdst channels.  The keywords are what the sites differ in:
        the output stride, the split-bf16 marker, the channel counts of a merged launch's destinations, and the non-NULL
        split-K fields (same split decision, hence the same partial-statistics row count, as the real launch)."""
        d.N, d.OH, d.OW, d.Cout, d.nsrc = dz.N, H, W, Cdst, 1
        sv = d.src[0]
        sv.C, sv.ldc, sv.H, sv.W = Kd, dz.ldc, dz.H, dz.W
        d.ntaps = len(sub)
        for i, (dy, dx, _) in enumerate(sub):
            d.tdy[i], d.tdx[i] = dy, dx
        d.in_stride, d.gather = 1, gather
        if out_stride:
            d.out_sy = d.out_sx = out_stride
        if w_s3:
            d.w_s3 = 1
        d.ndst = len(dst_C)
        for k, c in enumerate(dst_C):
            d.dst[k].C = c
        if splitk:
            d.splitk_ws, d.splitk_ws_bytes = 1, SPLITK_BYTES
            d.splitk_tickets = 1 if self.sk_fused else None

    def _dgrad_epilogue(self, e, s, tgt, acc, hook):
        """where and how an input-gradient launch writes the gradient of operand ``s``; ``e`` is the descriptor itself or one
        destination of a merged launch (pmf_conv_dst_t: the same field names).  accumulate / Dropout2d multiplier / ReLU
        mask of the operand's view / from a filled hook, the BatchNorm-backward partial sums (_arm_bn_carry)."""
        r = s.root()
        e.out, e.out_ldc, e.accumulate = tgt.buf.ptr, tgt.ldc, acc
        if s.cmul is not None:
            e.ep_cmul, e.ep_cmul_ld = self.masks_ptr + 4 * s.cmul, s.cmul_ld
        if r.relu:
            e.ep_relu_x, e.ep_relu_ldc = r.t.buf.ptr, r.t.ldc
            e.ep_relu_scale = r.scale.ptr if r.scale is not None else None
            e.ep_relu_shift = r.shift.ptr if r.shift is not None else None
        if hook:
            e.stats, e.ep_stat_mean = hook["rows"].ptr, hook["mean"].ptr
            if not r.relu:
                e.ep_relu_x, e.ep_relu_ldc, e.ep_flags = r.t.buf.ptr, r.t.ldc, L.EP_STAT_X_ONLY

    def _dgrad(self, srcs, conv, dz, taps, stride, gather, name):
        """input gradients: the same implicit-GEMM kernel run over dz with transposed weights.
        stride 1:  dX[y] = sum_t dz[y - dy_t] W_t^T                      (one launch per operand)
        stride 2:  y = 2m + py:  dX[y] = sum_{t: (py-dy_t) even} dz[m + (py-dy_t)/2] W_t^T   (one launch per parity)"""
        if not any(s.t.needs_grad for s in srcs):
            return
        if stride == 1:
            classes = [(0, 0, [(-dy, -dx, wi) for (dy, dx, wi) in taps])]
        else:
            classes = []
            for py in range(2):
                for px in range(2):
                    sub = [((py - dy) // 2, (px - dx) // 2, wi) for (dy, dx, wi) in taps
                           if (py - dy) % 2 == 0 and (px - dx) % 2 == 0]
                    if sub:
                        classes.append((py, px, sub))
        ldwT = _ru(sum(_ru(s.t.C, 8) for s in srcs), 64) + 64
        Kd, dg_s3, packs = self._dgrad_packs(srcs, conv, dz, classes, stride, gather, ldwT)
        if (stride == 1 and packs is not None and all(dg_s3)
                and self._dgrad_merged(srcs, conv, dz, Kd, gather, classes[0][2], packs[0], ldwT, name)):
            return
        coloff = 0
        for s in srcs:
            Cs = _ru(s.t.C, 8)
            if s.t.needs_grad:
                if packs is None:
                    own_ld = _ru(Cs, 64) + 64
                    own = [self.add_pack(conv.weight, [t[2] for t in sub], 1, Kd, own_ld, 1, cin=(coloff, Cs))
                           for (_, _, sub) in classes]
                    self._dgrad_operand(s, conv, dz, Kd, gather, stride, classes, dg_s3, own, own_ld, 0, name)
                else:
                    self._dgrad_operand(s, conv, dz, Kd, gather, stride, classes, dg_s3, packs, ldwT, coloff, name)
            coloff += Cs

    def _dgrad_packs(self, srcs, conv, dz, classes, stride, gather, ldwT):
        """(K of the input-gradient GEMM, per parity class whether it runs on the split-bf16 kernels, the transposed weight pack
        of every class -- or None: every operand gets packs of its own channel range, see below)"""
        Cout = conv.out_channels
        Kd = _ru(Cout, 8)                       # (padded channels of dz are zero)
        ref = next(s for s in srcs if s.t.needs_grad)

        def s3(Kd):
            return [Kd % 16 == 0 and self.s3_ok(lambda d: self._dgrad_shape(
                d, dz, Kd, gather, sub, *_class_hw(ref.t.H, ref.t.W, stride, py, px), ref.t.C)) for (py, px, sub) in classes]
        if Kd % 16 and self.s3:
            # 20 output channels (the logits heads): K = 24 keeps the launch off the split kernels.  Rounded up to 32 the last
            # eight "channels" of a pixel are the first eight of the next pixel (finite values; past the end of the tensor the
            # buffer range check returns 0) against weight rows that are zero -- they add exactly 0
            if all(s3(_ru(Cout, 16))):
                Kd = _ru(Cout, 16)
        dg_s3 = s3(Kd)
        # split-bf16 launches address the transposed weights by 32-column fragments: every operand that receives a
        # gradient must start on one
        offs, co_ = [], 0
        for s in srcs:
            offs.append(co_)
            co_ += _ru(s.t.C, 8)
        aligned = all(o % 32 == 0 for o, s in zip(offs, srcs) if s.t.needs_grad)
        # operands that do not start on a 32-column fragment (16 + 64 channels): every operand gets its own transposed
        # pack of its channel range, starting at column 0
        if not aligned and all(dg_s3) and all(_ru(s.t.C, 8) == s.t.C for s in srcs):
            return Kd, dg_s3, None
        if not aligned:
            dg_s3 = [False] * len(classes)
        return Kd, dg_s3, [self.add_pack(conv.weight, [t[2] for t in sub], 1, Kd, ldwT, int(k3))
                           for (_, _, sub), k3 in zip(classes, dg_s3)]

    def _dgrad_merged(self, srcs, conv, dz, Kd, gather, sub, wT, ldwT, name):
        """one launch for all operands of a concatenated input (stride 1, split-bf16 path, every operand a whole number of
        32-channel fragments): dz is read ONCE and the output-channel ranges go to the operands' gradient tensors, each
        with its own epilogue.  Returns False, with nothing allocated or emitted, where the launch does not apply."""
        if not (2 <= len(srcs) <= L.MAX_SRC and all(s.t.needs_grad and not s.bcast and s.t.C % 32 == 0 for s in srcs)
                and dz.N * dz.H * dz.W >= int(os.environ.get("PMF_DGRAD_MERGE_MINPIX", "1024"))
                and os.environ.get("PMF_DGRAD_MERGE", "1") != "0"):
            return False
        # torch.cat of one tensor (or one root) twice: two destinations would be ONE gradient buffer, written with
        # accumulate 0 and 1 by workgroups of one launch in unspecified order -- such a concat keeps the per-operand
        # launches (stream order)
        if len({id(s.root() if s.root().bn is not None else s.root().t) for s in srcs}) != len(srcs):
            return False
        H, W, chans = srcs[0].t.H, srcs[0].t.W, [s.t.C for s in srcs]

        def shape_only(d):
            self._dgrad_shape(d, dz, Kd, gather, sub, H, W, sum(chans), out_stride=1, w_s3=True, dst_C=chans)
        # the library's own eligibility rule, on the shape-only descriptor (a mismatch would otherwise only surface as
        # PMF_E_ARG when the plan runs) -- before grad_of, which allocates
        probe = L.ConvDesc()
        shape_only(probe)
        if not L.lib().pmf_conv_multi_ok(C.byref(probe)):
            return False
        dsts = [(s,) + self.grad_of(s) + ({},) for s in srcs]       # (operand, gradient tensor, accumulate, BN-carry hook)

        def f(op):
            d = op.u.conv
            shape_only(d)
            d.src[0].x = dz.buf.ptr
            d.ldw, d.w_s3, d.act = ldwT, wT.ptr, L.ACT_NONE
            d.out_H, d.out_W = H, W
            d.out, d.out_ldc = dsts[0][1].buf.ptr, dsts[0][1].ldc
            for k, dst in enumerate(dsts):
                self._dgrad_epilogue(d.dst[k], *dst)
        self.emit(self.bwd, L.OP_CONV, f)
        for s, tgt, _, hook in dsts:
            self._arm_bn_carry(s.root(), tgt, hook, shape_only)
        self.meta_bwd[len(self.bwd) - 1] = dict(
            family="conv_dgrad", flops=2.0 * dz.N * H * W * sum(chans) * conv.out_channels * len(sub), name=name,
            shape="%dx%dx%d %d->%s t%d s1" % (dz.N, H, W, conv.out_channels, "+".join(str(c) for c in chans), len(sub)))
        return True

    def _dgrad_operand(self, s, conv, dz, Kd, gather, stride, classes, dg_s3, packs, ldwT, coloff, name):
        """the input-gradient launches of ONE operand, one per parity class; its columns of the transposed packs start at
        ``coloff``"""
        r = s.root()
        if s.bcast:
            # 1x1 map broadcast over the image: full-size gradient into a temp, then per-sample column sums
            tmp = T(self, dz.N, dz.H, dz.W, s.t.C, name + ".bcast_tmp")
            if r.t.g is None:
                r.t.g = T(self, r.t.N, 1, 1, r.t.C, r.t.name + ".g", arena=self.zero_bwd, ldc=r.t.ldc)
            r.t.g_written = True
            self._touch(r.t.g)
            tgt, acc = tmp, 0
        else:
            tgt, acc = self.grad_of(s)
            if stride != 1:
                # parity classes only touch their own pixels: zero first, then accumulate
                if not acc:
                    self.fill(self.bwd, tgt.buf, tgt.npix * tgt.ldc)
                acc = 1
        for cls, wT, k3 in zip(classes, packs, dg_s3):
            self._dgrad_launch(s, tgt, acc, conv, dz, Kd, gather, stride, cls, wT, k3, ldwT, coloff, name)
        if s.bcast:
            g = r.t.g
            crows = self.act.alloc(COL_ROWS * tmp.N * _ru(g.ldc, 4) * 4)
            self.emit(self.bwd, L.OP_COLSUM, lambda op: _sm(
                op, p=(tmp.buf.ptr, g.buf.ptr, crows.ptr), i=(tmp.ldc, g.ldc, tmp.N), l=(tmp.H * tmp.W,)))

    def _dgrad_launch(self, s, tgt, acc, conv, dz, Kd, gather, stride, cls, wT, k3, ldwT, coloff, name):
        """one input-gradient launch: parity class ``cls`` of the gradient of operand ``s`` into ``tgt``"""
        (py, px, sub), lane, Cout = cls, self.lane, conv.out_channels
        mh, mw = _class_hw(tgt.H, tgt.W, stride, py, px)

        def shape_only(d):
            self._dgrad_shape(d, dz, Kd, gather, sub, mh, mw, s.t.C, out_stride=stride, w_s3=bool(k3), splitk=True)
        # filled in by the BatchNorm backward of the layer that produced this operand when THIS launch is the last
        # writer of its output gradient: the launch then also writes the BN-backward partial sums (_arm_bn_carry)
        hook = {}

        def f(op):
            d = op.u.conv
            shape_only(d)
            d.src[0].x = dz.buf.ptr
            d.ldw = ldwT
            if k3:      # fragment column coloff / 32 (3 planes x 1 KiB each)
                d.w_s3 = wT.ptr + (coloff // 32) * 3 * 1024
            else:
                d.w = wT.at(coloff)
            d.act = L.ACT_NONE
            d.out_H, d.out_W = tgt.H, tgt.W
            d.out_oy, d.out_ox = py, px
            d.splitk_ws, d.splitk_ws_bytes = self.sk_bufs[lane].ptr, self.sk_bufs[lane].nbytes
            d.splitk_tickets = self.sk_tickets[lane].ptr if self.sk_fused else None
            self._dgrad_epilogue(d, s, tgt, acc, hook)
        self.emit(self.bwd, L.OP_CONV, f)
        if stride == 1:
            self._arm_bn_carry(s.root(), tgt, hook, shape_only)
        self.meta_bwd[len(self.bwd) - 1] = dict(
            family="conv_dgrad", flops=2.0 * dz.N * mh * mw * s.t.C * Cout * len(sub), name=name,
            shape="%dx%dx%d %d->%d t%d s%d" % (dz.N, mh, mw, Cout, s.t.C, len(sub), stride))

    # ------------------------------------------------------------------ weight gradient
    def _wgrad(self, srcs, conv, dz, taps, stride, gather, name, dbias_rows=0, dbr=None, dbr_ld=0):
        Cout = conv.out_channels
        goff = self.pgrad(conv.weight)
        kh, kw = conv.kernel_size
        span = max(max(t[0] for t in taps) - min(t[0] for t in taps), max(t[1] for t in taps) - min(t[1] for t in taps))
        wg_gather = 1 if (gather or (3 * stride + 1 + span) * (31 * stride + 1 + span) * 128 > 100 * 1024) else 0

        def shape_fill(d):
            d.N, d.OH, d.OW, d.Cout, d.nsrc = dz.N, dz.H, dz.W, Cout, len(srcs)
            for i, s in enumerate(srcs):
                d.src[i].C = _ru(s.t.C, 8)
                d.src[i].ldc, d.src[i].H, d.src[i].W = s.t.ldc, s.t.H, s.t.W
            d.ntaps = len(taps)
            for i, (dy, dx, wi) in enumerate(taps):
                d.tdy[i], d.tdx[i], d.tap_widx[i] = dy, dx, wi
            d.in_stride, d.gather = stride, wg_gather
            d.Cin_real, d.KHW = conv.in_channels, kh * kw
        probe = L.WgradDesc()
        shape_fill(probe)
        probe.flags = L.WGRAD_S3 if self.s3 else 0       # (the kernel choice, hence the grid, depends on it)
        probe.nsplit = 1
        nsplit = L.lib().pmf_conv_wgrad_nsplit(C.byref(probe))
        probe.nsplit = nsplit
        self.wg_scratch = max(self.wg_scratch, L.lib().pmf_conv_wgrad_workspace(C.byref(probe)))

        def f(op):
            d = op.u.wgrad
            shape_fill(d)
            for i, s in enumerate(srcs):
                self.src_struct(s, d.src[i])
            d.dz, d.dz_ldc = dz.buf.ptr, dz.ldc
            d.partial = self.wg_bufs[lane].ptr
            d.nsplit = nsplit
            d.dw_oihw = self.pgrad_buf.at(goff)
            d.accumulate = 0
            d.flags = L.WGRAD_S3 if self.s3 else 0
            if dbias_rows:
                d.dbias_rows, d.dbias_nrows, d.dbias_ld = dbr.ptr, dbias_rows, dbr_ld
                d.dbias_out = self.pgrad_buf.at(boff)
        boff = self.pgrad(conv.bias) if dbias_rows else None
        home = self.lane
        lane = self._wgrad_lane_of(home) if (self.wgrad_lane and self._wgrad_lane_of(home) != home) else home
        self.n_wgrad += 1
        meta = dict(family="conv_wgrad", flops=2.0 * dz.N * dz.H * dz.W * Cout * conv.in_channels * len(taps), name=name,
                    shape="%dx%dx%d %d->%d t%d" % (dz.N, dz.H, dz.W, conv.in_channels, Cout, len(taps)))
        ws = None
        if self.flat is not None and self.batch_reds:
            # flat training state (the product path): the partial-slab kernel now, the reduction into OIHW later -- the
            # reductions of RED_BATCH consecutive layers are ONE launch (pmf_conv_wgrad_reduce_multi); every layer keeps
            # its own workspace until then (1.65 GB at 64x2048 bs 2: nothing next to 288 GB)
            ws = self.act.alloc(max(L.lib().pmf_conv_wgrad_workspace(C.byref(probe)), 256))

        def emit_ops():          # on the current lane
            if ws is not None:
                def fb(op):
                    f(op)
                    op.u.wgrad.partial = ws.ptr
                self.emit(self.bwd, L.OP_WGRAD_PART, fb)
                self.meta_bwd[len(self.bwd) - 1] = meta
                pend = self.pending_reds.setdefault(lane, [])
                pend.append((fb, [conv.weight] + ([conv.bias] if dbias_rows else [])))
                if len(pend) >= self.red_batch:
                    self.flush_reds(lane)
            else:
                # per-tensor gradients (tests, stock DistributedDataParallel): partial slabs, then the reduction into
                # OIHW, back to back on the op's lane through that lane's workspace
                self.emit(self.bwd, L.OP_WGRAD_PART, f)
                self.meta_bwd[len(self.bwd) - 1] = meta
                self.emit(self.bwd, L.OP_WGRAD_RED, f)
                self.grad_done[id(conv.weight)] = len(self.bwd) - 1
                if dbias_rows:
                    self.grad_done[id(conv.bias)] = len(self.bwd) - 1
        if lane == home:
            emit_ops()
        else:
            # weight-gradient lane: the ops are DEFERRED and emitted in batches behind ONE event of the home lane (every
            # dz stays alive in the arena until the end of the pass, so running a weight gradient late is always legal)
            q = self._wg_deferred.setdefault(home, [])
            q.append(emit_ops)
            if len(q) >= self.wgrad_batch:
                self.flush_wgrads(home)

    def flush_wgrads(self, home):
        q = self._wg_deferred.pop(home, [])
        if not q:
            return
        ready = self.record_event(self.bwd, lane=home)      # everything the batch reads is complete after this op
        self._emit_batch(home, q, ready)

    def _emit_batch(self, home, q, ready):
        prev = self.lane
        self.lane = self._wgrad_lane_of(home)
        self.wait_event(self.bwd, ready)
        for fn in q:
            fn()
        self.lane = prev

    def flush_reds(self, lane):
        """emit ONE stage-2 launch for the weight gradients queued on ``lane`` by _wgrad (flat training state only)"""
        pend = self.pending_reds.pop(lane, [])
        if not pend:
            return
        prev, self.lane = self.lane, lane

        def f(op):
            lib = L.lib()
            n = len(pend)
            descs = (L.WgradDesc * n)()
            meta = (C.c_int32 * (8 * n))()
            tmp = L.Op()
            blocks = 0
            for j, (fill, _) in enumerate(pend):
                C.memset(C.addressof(tmp), 0, C.sizeof(tmp))      # fills only set what they use (as on a fresh op)
                fill(tmp)
                C.memmove(C.addressof(descs[j]), C.addressof(tmp.u.wgrad), C.sizeof(L.WgradDesc))
                row = (C.c_int32 * 8)()
                nb = lib.pmf_conv_wgrad_reduce_plan(C.byref(descs[j]), row)
                if nb <= 0:
                    raise RuntimeError("pmf_conv_wgrad_reduce_plan failed: %d" % nb)
                row[0] = blocks
                meta[8 * j:8 * j + 8] = row[:]
                blocks += nb
            jd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(self.device)
            md = torch.frombuffer(bytearray(bytes(meta)), dtype=torch.uint8).to(self.device)
            self._red_tables.append((jd, md))                  # keep the device tables alive with the plan
            _sm(op, p=(jd.data_ptr(), md.data_ptr()), i=(n, blocks))
        self.emit(self.bwd, L.OP_WGRAD_RED_MULTI, f)
        # data parallelism: the gradients this launch finalises (and everything listed before it) may be all-reduced as
        # soon as it AND the ops emitted so far on the two home lanes have run -- one event each; the engine makes its RCCL
        # side stream wait for them (pmf_plan_event_wait), no cut through the plan
        evs = [self._event_after(self._last_op[(id(self.bwd), lane)])[0]]
        for hl in (0, 1):
            ev = self.record_event(self.bwd, lane=hl)
            if ev is not None:
                evs.append(ev[0])
        self.dp_events.append((len(self.bwd), evs))
        self.lane = prev
        for _, params in pend:
            for p in params:
                self.grad_done[id(p)] = len(self.bwd) - 1
