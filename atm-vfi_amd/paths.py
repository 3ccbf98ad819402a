"""The stages of ``Network.forward``, lowered once per regime (DESIGN.md "Frame stage / pair stage").  ``Network._path`` makes one
object per eager forward, bound to ``(net, ops, P)``, by the one switch ``Network._plane_convs(ops)``:

* ``PlanesPath`` -- "f16x3" / "f16" with at most 2^26 plane rows (every benchmark configuration): all contractions read and write split
  planes; ``_PMap`` and ``Planes`` travel between its stages;
* ``RowsPath`` -- "f32", the tests' CPU double, and batches beyond 2^26 plane rows: fp32 NHWC rows travel between its stages.  In the
  last case its ``plane_deconvs`` flag is set and the decoder's deconvs read split planes (the "mixed" regime: a flag, not a class).

Both implement the same stages and the skeletons in ``network.py`` call them.  A new fused launch goes into the stage of the path it
belongs to; the other path never sees it.
"""
from __future__ import annotations

from typing import Optional


def _r4(c: int) -> int:
    return (c + 3) // 4 * 4


class _PMap:
    """A feature map that lives in split planes only: channels [32 * chunk0, 32 * chunk0 + c) of ``p``, rows = pixels of [n, h, w]."""
    __slots__ = ("p", "n", "h", "w", "chunk0", "c")

    def __init__(self, p, n, h, w, chunk0, c):
        self.p, self.n, self.h, self.w, self.chunk0, self.c = p, n, h, w, chunk0, c


class _Path:
    def __init__(self, net, ops, P):
        self.ops, self.P, self.v = ops, P, net._v
        self.buf, self.planes = net.buf, net.planes          # the workspace of the forward that made this object

    def wbp(self, p, act=True, wkey=None):
        """(packed weight, bias, PReLU slopes) of the reference's conv() / deconv() ``p`` (``p.0`` + ``p.1``), or without ``act`` of a
        bare nn.Conv2d ``p``."""
        P = self.P
        return (P[wkey or f"pk:{p}.0.weight"], P[f"{p}.0.bias"], P[f"{p}.1.weight"]) if act else (P[wkey or f"pk:{p}.weight"], P[f"{p}.bias"], None)

    def _skips(self, b, H, W):
        """The U-Net's fp32 skip buffers, which the rows path's decoder writes into: bufC [feat2_ | feat2 | dec0] at H/4, bufB [feat1_ | feat1 | dec1]
        at H/2, bufA [feat0_ | feat0] and the refiner's input [dec2 | im0 I0 im1 I1 It] at H."""
        rh = self.v.refine_hidden
        w1d, w2d, _ = self.v.decoder_widths
        return (self.buf("bufC", b, H // 4, W // 4, 4 * rh + _r4(w1d + 5)), self.buf("bufB", b, H // 2, W // 2, 2 * rh + _r4(w2d + 5)),
                self.buf("bufA", b, H, W, 2 * rh), self.buf("refine_in", b, H, W, self.v.refine_in))


class PlanesPath(_Path):
    """Split planes between all contractions; fp32 copies only where something other than a contraction reads them."""

    def c3p(self, p, xp, n, h, w, out=None, act=True, sink=None, sink_c0=0, sink_prelu=None, wkey=None, out_cmin=0, sink2=None):
        """conv()/Conv2d 3x3 s1 p1 of the reference on split-plane input ``xp`` ([n*h*w rows])."""
        wt, bias, prelu = self.wbp(p, act, wkey)
        extra = {} if sink2 is None else {"planes2": sink2}
        # under-filled grids with long K (the motion MLPs of small frames): split K over the idle CUs; the scratch for the partial
        # sums is workspace memory like every other buffer
        need = self.ops.conv3x3_workspace_floats(n, h, w, wt.cin, wt.cout)
        if need:
            extra["workspace"] = self.buf("splitk_ws", need)
        self.ops.conv3x3_planes(xp, n, h, w, wt, out=out, bias=bias, prelu=prelu, planes=sink, planes_c0=sink_c0, planes_prelu=sink_prelu,
                                out_cmin=out_cmin, **extra)

    def conv_p(self, p, src: _PMap, stride=1, pad=1, dil=1, act=True, out=None, sink=None, sink_c0=0, src2: Optional[_PMap] = None):
        """conv() / nn.Conv2d of the reference (any stride / dilation, k 1 or 3) on a split-plane map through the LDS-DMA GEMM."""
        wt, bias, prelu = self.wbp(p, act)
        two = {} if src2 is None else {"x2": src2.p, "x2_chunk0": src2.chunk0, "split_chunks": src.c // 32}
        self.ops.conv_planes(src.p, src.n, src.h, src.w, wt, out=out, stride=stride, pad=pad, dil=dil, bias=bias, prelu=prelu, sink=sink,
                             sink_c0=sink_c0, in_chunk0=src.chunk0, **two)

    def deconv(self, p, xp, sink, in_shape):
        """deconv() of the reference, split planes in and out (LDS-DMA GEMM)."""
        wt, bias, prelu = self.wbp(p)
        self.ops.deconv(None, wt, None, bias=bias, prelu=prelu, planes=xp, sink=sink, in_shape=in_shape)

    # ---- the frame stage: encoder, fusion, global_tokens -- and, directly below them, the split-K mirror of their launches ----
    def encoder(self, x0, tag: str):
        """shared_feat_extraction (network_base.py:342-352).  x0: [F,H,W,4].  Returns (e1, e2, fuse_l) as ``_PMap`` (no fp32 copy exists:
        their only readers are contractions), s3 already in the last channels of fuse_l's planes.  The full-resolution stem (3 -> d0
        -> d0 -> d1 stride 2) is ONE launch whose two d0-channel maps stay in LDS; then stride-2 conv (LDS-DMA GEMM, CONV mode) ->
        planes -> 3x3 conv (plane kernel) -> planes per stage."""
        d, ld = self.v.hidden_dims, self.v.local_dim
        f, h, w, _ = x0.shape
        fuse_p = self.planes(f"{tag}fuse_l_p", f * (h // 8) * (w // 8), ld)
        src, outs = None, []
        for st in (1, 2, 3):
            hs, ws = h >> st, w >> st
            ap = self.planes(f"{tag}e{st}a_p", f * hs * ws, d[st])
            if st == 1:
                self.ops.stem_fused(x0, self.P["stem"], ap)
            else:
                self.conv_p(f"feat_extracts.{st}.0", src, stride=2, sink=ap)
            if st == 3:
                self.c3p("feat_extracts.3.1", ap, f, hs, ws, sink=fuse_p, sink_c0=ld - d[3])
                outs.append(_PMap(fuse_p, f, hs, ws, 0, ld))
            else:
                ep = self.planes(f"{tag}e{st}_p", f * hs * ws, d[st])
                self.c3p(f"feat_extracts.{st}.1", ap, f, hs, ws, sink=ep)
                outs.append(_PMap(ep, f, hs, ws, 0, d[st]))
                src = outs[-1]
        return outs[0], outs[1], outs[2]

    def fusion(self, p, fine: _PMap, mid: _PMap, fuse: _PMap, c_mid, c_fine, tag):
        """CrossScaleFeatureFusion (network_base.py:73-85); the coarsest scale is already in fuse's planes and the three strided convs
        sink next to it; the 1x1 projection is the LDS-DMA GEMM on those planes (no fp32 fusion buffer).  Returns LayerNorm'ed tokens
        [F*h*w, C] (fp32: the blocks' first LayerNorm gathers them)."""
        P, ops = self.P, self.ops
        f, h, w, c = fuse.n, fuse.h, fuse.w, fuse.c
        self.conv_p(f"{p}.layers.0", mid, stride=2, pad=1, dil=1, act=False, sink=fuse.p, sink_c0=0)
        self.conv_p(f"{p}.layers.1", fine, stride=4, pad=1, dil=1, act=False, sink=fuse.p, sink_c0=c_mid)
        self.conv_p(f"{p}.layers.2", fine, stride=4, pad=2, dil=2, act=False, sink=fuse.p, sink_c0=c_mid + c_fine)
        t = self.buf(f"{tag}fproj", f * h * w, c)
        ops.linear(fuse.p, P[f"pk:{p}.proj.weight"], t, bias=P[f"{p}.proj.bias"])
        out = self.buf(f"{tag}fnorm", f * h * w, c)
        ops.layernorm(t, out, P[f"{p}.norm.weight"], P[f"{p}.norm.bias"])
        return out

    def global_tokens(self, e2: _PMap, fuse_l: _PMap, tag):
        """The per-frame half of estimate_global_motion (network_base.py:391-400): last_feat_extract + the global cross-scale fusion.
        Returns the LayerNorm'ed tokens [F*h_*w_, global_dim] of the F frames in ``e2`` / ``fuse_l``."""
        v = self.v
        d = v.hidden_dims
        f, h8, w8 = fuse_l.n, fuse_l.h, fuse_l.w
        h_, w_ = h8 // 2, w8 // 2
        s3 = _PMap(fuse_l.p, f, h8, w8, (v.local_dim - d[3]) // 32, d[3])
        fuse_g = _PMap(self.planes(f"{tag}fuse_g_p", f * h_ * w_, v.global_dim), f, h_, w_, 0, v.global_dim)
        ap = self.planes(f"{tag}ga_p", f * h_ * w_, v.last_feat_dim)
        self.conv_p("last_feat_extract.0", s3, stride=2, sink=ap)
        self.c3p("last_feat_extract.1", ap, f, h_, w_, sink=fuse_g.p, sink_c0=d[3] + 2 * d[2])
        return self.fusion("global_feature_fusion", e2, s3, fuse_g, d[3], d[2], tag + "g")

    @staticmethod
    def frame_stage_splitk(net, ops, H: int, W: int, f: int, glob: bool):
        """MIRROR of the three methods above: the split-K factors the library would choose for their contraction launches on ``f``
        frames of H x W, in launch order (``encoder``; ``fusion``; with ``glob``, ``global_tokens`` and its ``fusion``).  A launch added
        to, removed from or reordered in one of the three changes this list in the same edit.  Under-filled grids with long K are cut
        over the idle CUs (``gemm_splitk_plan``, ``conv3_plan``: host-side functions of the launch's ROWS), and a different cut sums in
        a different order: tokens are bit-identical to ``forward``'s only when computed under the same factors."""
        v = net._v
        d = v.hidden_dims
        c32 = lambda c: (c + 31) // 32

        def gemm(rows, cout, cin, taps=9):
            if ops.gemm_workspace is None:
                return 1
            need = int(ops.lib.atmvfi_gemm_workspace_floats(rows, cout, taps * c32(cin)))
            return need // (rows * ((cout + 63) // 64 * 64)) if need else 1

        def c3(h, w, cin, cout):
            need = ops.conv3x3_workspace_floats(f, h, w, cin, cout)
            return need // (f * h * w * ((cout + 15) // 16 * 16)) if need else 1
        out = []
        for st in (1, 2, 3):
            hs, ws = H >> st, W >> st
            if st > 1:
                out.append(gemm(f * hs * ws, d[st], d[st - 1]))                   # feat_extracts.st.0 (stride 2)
            out.append(c3(hs, ws, d[st], d[st]))                                   # feat_extracts.st.1
        h, w = H // 8, W // 8
        out += [gemm(f * h * w, d[2], d[2]), gemm(f * h * w, d[1], d[1]), gemm(f * h * w, d[1], d[1]),      # fusion layers 0..2
                gemm(f * h * w, v.local_dim, v.local_dim, 1)]                                                  # fusion projection
        if glob:
            h_, w_ = H // 16, W // 16
            out += [gemm(f * h_ * w_, v.last_feat_dim, d[3]), c3(h_, w_, v.last_feat_dim, v.last_feat_dim),    # last_feat_extract
                    gemm(f * h_ * w_, d[3], d[3]), gemm(f * h_ * w_, d[2], d[2]), gemm(f * h_ * w_, d[2], d[2]),
                    gemm(f * h_ * w_, v.global_dim, v.global_dim, 1)]
        return tuple(out)

    # ---- the pair stage ----
    def motion_sinks(self, tag, rows, cin, c):
        """Per ATMFormer block of a motion branch, (``out_sink``, ``motion_sink``) of ``BlockRunner._block``: the motion MLP's input
        [motion 8 | frame0 C | frame1 C] is assembled as split planes by its producers -- the four motion channels of block ``blk``
        (frame 0 dx dy, frame 1 dx dy at 4 blk ..) straight from the motion head, the features from the second block's fc2."""
        mlp_in_p = self.planes(f"{tag}mlp_in_p", rows, cin)
        return (None, (mlp_in_p, 0, 2)), ((mlp_in_p, 8, c), (mlp_in_p, 4, 2))

    def motion_mlp(self, mlp, mlp_in, b, h, w, tag):
        """The two 3x3 convs of a motion MLP after the two ATMFormer blocks, on the planes ``motion_sinks`` named.  -> hidden Planes."""
        hid = self.P[f"{mlp}.0.0.bias"].shape[0]
        mlp_in_p = self.planes(f"{tag}mlp_in_p", b * h * w, mlp_in.shape[-1])
        t1p = self.planes(f"{tag}mm1_p", b * h * w, hid)
        t2p = self.planes(f"{tag}mm2_p", b * h * w, hid)
        self.c3p(f"{mlp}.0", mlp_in_p, b, h, w, sink=t1p)
        self.c3p(f"{mlp}.1", t1p, b, h, w, sink=t2p)
        return t2p

    def head1x1(self, p, t2, b, h, w, out):
        """The 1x1 head of a motion MLP (network_base.py:158,195) on the hidden map's planes: 5 channels, a lane per pixel, no GEMM tile."""
        self.ops.head1x1_planes(t2, b, h, w, self.P[f"pk:{p}.weight"], out, bias=self.P[f"{p}.bias"])

    def _refine_in_p(self, b, H, W):
        """The refiner's input planes [dec2 (w3+5) | zeros to the next multiple of 8 | 15 image channels] and where the 15 start."""
        pack_c0 = (self.v.decoder_widths[2] + 5 + 7) // 8 * 8
        return self.planes("refine_in_p", b * H * W, pack_c0 + 15), pack_c0

    def decoder_input(self, x, b, H, W):
        """``x`` [b,h,w,cdec] fp32 (two warps and a 1x1 head wrote it): one split pass.  -> the Planes stage 0's deconv reads."""
        # the rows path's fp32 skip buffers: nothing here reads or writes them, but the workspace's size is part of what a forward
        # is pinned to (workspace_bytes()); dropping them is a change of its own
        self._skips(b, H, W)
        xp = self.planes("dec_xp_0", x.shape[0] * x.shape[1] * x.shape[2], x.shape[3])
        self.ops.split_planes(x.flatten(0, 2), xp)
        return xp

    def decoder_stage(self, st, xp, b, hs, wsz):
        """Decoder stage ``st`` (network_base.py:511-528) at hs x wsz, planes end to end: deconv (LDS-DMA GEMM) -> planes -> conv+PReLU
        -> planes -> conv -> planes for the next stage (through its leading PReLU) or for the refiner's first conv.  fp32 only for the
        five flow / mask channels that warp_blend reads (in a compact 8-float-per-pixel buffer: as the tail of a 400-600-byte row each
        pixel's 20 bytes would cost warp_blend a cache line of their own).  -> (the next stage's input Planes or None, that map)."""
        P = self.P
        pfx, o = f"upsample_pyramid.{st}", 1 if st else 0
        cout = self.v.decoder_widths[st] + 5
        t1p = self.planes(f"dec_t1_{st}_p", b * hs * wsz, cout)
        self.deconv(f"{pfx}.{o}", xp, t1p, (b, hs // 2, wsz // 2, xp.c))
        t2p = self.planes(f"dec_t2_{st}_p", b * hs * wsz, cout)
        self.c3p(f"{pfx}.{o + 1}", t1p, b, hs, wsz, sink=t2p)
        cmin = (cout - 5) // 4 * 4
        mot_c = self.buf(f"dec_mot_{st}", b, hs, wsz, 8)[..., :cout - cmin]
        if st < 2:
            # the map goes on twice as planes -- through the next stage's leading PReLU (its deconv) and raw (the U-Net's strided
            # conv reads cat(feat, dec[:, :w]) from two plane buffers)
            xp_next = self.planes(f"dec_xp_{st + 1}", b * hs * wsz, cout)
            raw = self.planes(f"dec_raw_{st}", b * hs * wsz, cout)
            self.c3p(f"{pfx}.{o + 2}", t2p, b, hs, wsz, out=mot_c, act=False, sink=xp_next, sink_prelu=P[f"inprelu:{st + 1}"], sink2=raw,
                     out_cmin=cmin)
        else:
            # finest level: the features go on to the refiner as planes
            xp_next = None
            self.c3p(f"{pfx}.{o + 2}", t2p, b, hs, wsz, out=mot_c, act=False, sink=self._refine_in_p(b, hs, wsz)[0], out_cmin=cmin)
        return xp_next, mot_c[..., mot_c.shape[-1] - 5:]

    def blend_pack(self, b, H, W):
        """Where the full-resolution warp_blend packs its 15 image channels for the refiner: into the refiner's input planes."""
        rin_p, pack_c0 = self._refine_in_p(b, H, W)
        return {"pack15": None, "pack_planes": rin_p, "pack_c0": pack_c0}

    def refiner(self, b, H, W, it0):
        """The residual refinement U-Net with its tail (network_base.py:417-431, 530-535).  -> (it0 + residual, the same clamped).
        feat0 / feat1 / feat2 exist as planes only (chunks of bufA_p / bufB_p / bufC_p): their readers are the strided convs (CONV mode
        of the ping-pong GEMM, two plane sources for the concats) and the up-path's 3x3 convs.  The first source (feat) ends on a
        32-channel chunk boundary; the second (dec[:, :w]) may end inside a chunk -- what follows there in the raw decoder planes (its
        flow / mask channels, then zeros) meets zero-padded weight channels."""
        P, ops = self.P, self.ops
        rh = self.v.refine_hidden
        w1d, w2d, _ = self.v.decoder_widths
        h, w, h2, w2, h4, w4 = H // 8, W // 8, H // 2, W // 2, H // 4, W // 4
        rin_p, _ = self._refine_in_p(b, H, W)
        bufA_p = self.planes("bufA_p", b * H * W, 2 * rh)                  # [up3 out | feat0]
        bufB_p = self.planes("bufB_p", b * h2 * w2, 2 * rh)                # [up2 out | feat1]
        bufC_p = self.planes("bufC_p", b * h4 * w4, 4 * rh)                # [up1 out | feat2]
        d2a_p = self.planes("d2a_p", b * h4 * w4, 2 * rh)
        d3a_p = self.planes("d3a_p", b * h * w, 4 * rh)
        self.c3p("proj", rin_p, b, H, W, sink=bufA_p, sink_c0=rh, wkey="pk:proj.0.weight:planes")
        self.conv_p("down1.0", _PMap(bufA_p, b, H, W, rh // 32, rh), stride=2, sink=bufB_p, sink_c0=rh)
        self.conv_p("down2.0", _PMap(bufB_p, b, h2, w2, rh // 32, rh), stride=2, sink=d2a_p,
                    src2=_PMap(self.planes("dec_raw_1", b * h2 * w2, w2d + 5), b, h2, w2, 0, w2d))
        self.c3p("down2.1", d2a_p, b, h4, w4, sink=bufC_p, sink_c0=2 * rh)
        self.conv_p("down3.0", _PMap(bufC_p, b, h4, w4, 2 * rh // 32, 2 * rh), stride=2, sink=d3a_p,
                    src2=_PMap(self.planes("dec_raw_0", b * h4 * w4, w1d + 5), b, h4, w4, 0, w1d))
        d3b_p = self.planes("d3b_p", b * h * w, 4 * rh)
        self.c3p("down3.1", d3a_p, b, h, w, sink=d3b_p)
        d3c_p = self.planes("d3c_p", b * h * w, 4 * rh)
        self.c3p("down3.2", d3b_p, b, h, w, sink=d3c_p)
        u1a_p = self.planes("u1a_p", b * h4 * w4, 2 * rh)
        self.deconv("up1.0", d3c_p, u1a_p, (b, h, w, 4 * rh))
        self.c3p("up1.1", u1a_p, b, h4, w4, sink=bufC_p, sink_c0=0)
        u2a_p = self.planes("u2a_p", b * h2 * w2, 2 * rh)
        self.deconv("up2.0", bufC_p, u2a_p, (b, h4, w4, 4 * rh))
        self.c3p("up2.1", u2a_p, b, h2, w2, sink=bufB_p, sink_c0=0)
        self.deconv("up3.0", bufB_p, bufA_p, (b, h2, w2, 2 * rh))
        # refine_head.0 -> refine_head.1 -> 2 sigmoid - 1 -> += -> clamp in two launches; the 64-channel full-resolution map r1 never
        # reaches HBM: the first launch leaves 27 "tap contributions" per pixel, the second adds the nine shifted ones of every output
        # pixel (include/atmvfi.h, atmvfi_conv3p_params: the fused read-out)
        contrib = self.buf("tail_contrib", 27, b * H * W)
        ops.conv3x3_planes_readout(bufA_p, b, H, W, P["pk:refine_head.0.0.weight"], P["refine_head.0.0.bias"],
                                   P["refine_head.0.1.weight"], P["readout"], contrib)
        it_sum, it_final = ops.empty(b, 3, H, W), ops.empty(b, 3, H, W)
        ops.refine_tail(contrib, P["refine_head.1.0.bias"], P["refine_head.1.1.weight"], it0, it_sum, it_final)
        return it_sum, it_final


class RowsPath(_Path):
    """fp32 NHWC rows between all stages.  ``plane_deconvs``: the decoder's deconvs read split planes all the same (the backend has
    the f16x3 plane engine; the batch's rows do not fit the plane kernels' 32-bit offsets)."""

    def __init__(self, net, ops, P):
        super().__init__(net, ops, P)
        self.plane_deconvs = net._plane_deconvs(ops)

    def conv_act(self, p, x, out, stride=1):
        wt, bias, prelu = self.wbp(p)
        self.ops.conv(x, wt, out, stride=stride, pad=1, dil=1, bias=bias, prelu=prelu)

    def conv_plain(self, p, x, out, stride=1, pad=1, dil=1, **planes):
        wt, bias, _ = self.wbp(p, act=False)
        self.ops.conv(x, wt, out, stride=stride, pad=pad, dil=dil, bias=bias, **planes)

    def deconv_act(self, p, x, out, **how):
        wt, bias, prelu = self.wbp(p)
        self.ops.deconv(x, wt, out, bias=bias, prelu=prelu, **how)

    # ---- the frame stage ----
    def encoder(self, x0, tag: str):
        """shared_feat_extraction (network_base.py:342-352).  x0: [F,H,W,4].  Returns (e1, e2, fuse_l), s3 already in fuse_l[..., -d3:]."""
        d, ld = self.v.hidden_dims, self.v.local_dim
        f, h, w, _ = x0.shape
        a = self.buf(f"{tag}e0a", f, h, w, d[0]); self.conv_act("feat_extracts.0.0", x0[..., :3], a)
        e0 = self.buf(f"{tag}e0", f, h, w, d[0]); self.conv_act("feat_extracts.0.1", a, e0)
        a = self.buf(f"{tag}e1a", f, h // 2, w // 2, d[1]); self.conv_act("feat_extracts.1.0", e0, a, 2)
        e1 = self.buf(f"{tag}e1", f, h // 2, w // 2, d[1]); self.conv_act("feat_extracts.1.1", a, e1)
        a = self.buf(f"{tag}e2a", f, h // 4, w // 4, d[2]); self.conv_act("feat_extracts.2.0", e1, a, 2)
        e2 = self.buf(f"{tag}e2", f, h // 4, w // 4, d[2]); self.conv_act("feat_extracts.2.1", a, e2)
        a = self.buf(f"{tag}e3a", f, h // 8, w // 8, d[3]); self.conv_act("feat_extracts.3.0", e2, a, 2)
        fuse = self.buf(f"{tag}fuse_l", f, h // 8, w // 8, ld)
        self.conv_act("feat_extracts.3.1", a, fuse[..., ld - d[3]:])
        return e1, e2, fuse

    def fusion(self, p, fine, mid, fuse, c_mid, c_fine, tag):
        """CrossScaleFeatureFusion (network_base.py:73-85); the coarsest scale is already in fuse[..., c_mid+2*c_fine:].  -> tokens."""
        P, ops = self.P, self.ops
        f, h, w, c = fuse.shape
        self.conv_plain(f"{p}.layers.0", mid, fuse[..., 0:c_mid], stride=2, pad=1, dil=1)
        self.conv_plain(f"{p}.layers.1", fine, fuse[..., c_mid:c_mid + c_fine], stride=4, pad=1, dil=1)
        self.conv_plain(f"{p}.layers.2", fine, fuse[..., c_mid + c_fine:c_mid + 2 * c_fine], stride=4, pad=2, dil=2)
        t = self.buf(f"{tag}fproj", f * h * w, c)
        ops.linear(fuse.reshape(f * h * w, c), P[f"pk:{p}.proj.weight"], t, bias=P[f"{p}.proj.bias"])
        out = self.buf(f"{tag}fnorm", f * h * w, c)
        ops.layernorm(t, out, P[f"{p}.norm.weight"], P[f"{p}.norm.bias"])
        return out

    def global_tokens(self, e2, fuse_l, tag):
        """The per-frame half of estimate_global_motion (network_base.py:391-400), as ``PlanesPath.global_tokens``."""
        v = self.v
        d = v.hidden_dims
        f, h8, w8, _ = fuse_l.shape
        h_, w_ = h8 // 2, w8 // 2
        s3 = fuse_l[..., v.local_dim - d[3]:]
        fuse_g = self.buf(f"{tag}fuse_g", f, h_, w_, v.global_dim)
        a = self.buf(f"{tag}ga", f, h_, w_, v.last_feat_dim)
        self.conv_act("last_feat_extract.0", s3, a, 2)
        self.conv_act("last_feat_extract.1", a, fuse_g[..., d[3] + 2 * d[2]:])
        return self.fusion("global_feature_fusion", e2, s3, fuse_g, d[3], d[2], tag + "g")

    # ---- the pair stage ----
    def motion_sinks(self, tag, rows, cin, c):
        """As ``PlanesPath.motion_sinks``: none, the motion MLP reads the fp32 rows the blocks write."""
        return (None, None), (None, None)

    def motion_mlp(self, mlp, mlp_in, b, h, w, tag):
        """The two 3x3 convs of a motion MLP after the two ATMFormer blocks.  -> the hidden map [b,h,w,hid]."""
        hid = self.P[f"{mlp}.0.0.bias"].shape[0]
        t1 = self.buf(f"{tag}mm1", b, h, w, hid); self.conv_act(f"{mlp}.0", mlp_in, t1)
        t2 = self.buf(f"{tag}mm2", b, h, w, hid); self.conv_act(f"{mlp}.1", t1, t2)
        return t2

    def head1x1(self, p, t2, b, h, w, out):
        """The 1x1 head of a motion MLP (network_base.py:158,195)."""
        self.conv_plain(p, t2, out, pad=0)

    def decoder_input(self, x, b, H, W):
        """-> (the decoder's fp32 input, no planes of it yet: stage 0's input has several producers)."""
        return x, None

    def decoder_stage(self, st, x, b, hs, wsz):
        """Decoder stage ``st`` (network_base.py:511-528) at hs x wsz, writing into the U-Net's skip buffers.  ``x``: (the fp32 input
        map, its rows as split planes through this stage's leading PReLU or None).  -> (that pair for the next stage, the five flow /
        mask channels).  With ``plane_deconvs`` the deconvs run on the LDS-DMA GEMM from split planes (the fp32-input engine redoes the
        split once per column block, 7x for 389 -> 4*197): stage 0 gets them from one split pass, stages 1-2 from the epilogue of the
        3x3 conv that produces their input."""
        P = self.P
        x, xp = x
        pfx, o = f"upsample_pyramid.{st}", 1 if st else 0
        rh, cout = self.v.refine_hidden, self.v.decoder_widths[st] + 5
        skips = self._skips(b, hs << (2 - st), wsz << (2 - st))
        dst = (skips[0][..., 4 * rh:4 * rh + cout], skips[1][..., 2 * rh:2 * rh + cout], skips[3][..., 0:cout])[st]
        t1 = self.buf(f"dec_t1_{st}", b, hs, wsz, _r4(cout))[..., :cout]
        if self.plane_deconvs and st == 0 and self.wbp(f"{pfx}.{o}")[0].hi is not None:
            xp = self.planes("dec_xp_0", b * (hs // 2) * (wsz // 2), x.shape[-1])
            self.ops.split_planes(x.flatten(0, 2), xp)
        if xp is not None:
            self.deconv_act(f"{pfx}.{o}", x, t1, planes=xp)
        else:
            self.deconv_act(f"{pfx}.{o}", x, t1, in_prelu=P[f"inprelu:{st}"] if st else None)
        t2 = self.buf(f"dec_t2_{st}", b, hs, wsz, _r4(cout))[..., :cout]
        self.conv_act(f"{pfx}.{o + 1}", t1, t2)
        if self.plane_deconvs and st < 2:
            # the 3x3 epilogue also writes the split planes the next deconv reads
            xp = self.planes(f"dec_xp_{st + 1}", b * hs * wsz, cout)
            self.conv_plain(f"{pfx}.{o + 2}", t2, dst, planes=xp, planes_prelu=P[f"inprelu:{st + 1}"])
        else:
            xp = None
            self.conv_plain(f"{pfx}.{o + 2}", t2, dst)
        return (dst, xp), dst[..., cout - 5:cout]

    def blend_pack(self, b, H, W):
        """Where the full-resolution warp_blend packs its 15 image channels for the refiner: behind dec2 in the refiner's input."""
        w3 = self.v.decoder_widths[2] + 5
        return {"pack15": self._skips(b, H, W)[3][..., w3:w3 + 15]}

    def refiner(self, b, H, W, it0):
        """The residual refinement U-Net with its tail (network_base.py:417-431, 530-535).  -> (it0 + residual, the same clamped)."""
        ops = self.ops
        rh = self.v.refine_hidden
        w1d, w2d, _ = self.v.decoder_widths
        h, w = H // 8, W // 8
        bufC, bufB, bufA, rin = self._skips(b, H, W)
        r1 = self.buf("r1", b, H, W, rh)
        feat0 = bufA[..., rh:2 * rh]; self.conv_act("proj", rin, feat0)
        feat1 = bufB[..., rh:2 * rh]; self.conv_act("down1.0", feat0, feat1, 2)
        d2a = self.buf("d2a", b, H // 4, W // 4, 2 * rh); self.conv_act("down2.0", bufB[..., rh:2 * rh + w2d], d2a, 2)
        feat2 = bufC[..., 2 * rh:4 * rh]; self.conv_act("down2.1", d2a, feat2)
        d3a = self.buf("d3a", b, h, w, 4 * rh); self.conv_act("down3.0", bufC[..., 2 * rh:4 * rh + w1d], d3a, 2)
        d3b = self.buf("d3b", b, h, w, 4 * rh); self.conv_act("down3.1", d3a, d3b)
        feat3 = self.buf("d3c", b, h, w, 4 * rh); self.conv_act("down3.2", d3b, feat3)
        u1a = self.buf("u1a", b, H // 4, W // 4, 2 * rh); self.deconv_act("up1.0", feat3, u1a)
        self.conv_act("up1.1", u1a, bufC[..., 0:2 * rh])
        u2a = self.buf("u2a", b, H // 2, W // 2, 2 * rh); self.deconv_act("up2.0", bufC[..., 0:4 * rh], u2a)
        self.conv_act("up2.1", u2a, bufB[..., 0:rh])
        self.deconv_act("up3.0", bufB[..., 0:2 * rh], bufA[..., 0:rh])
        self.conv_act("refine_head.0", bufA, r1)
        it_sum, it_final = ops.empty(b, 3, H, W), ops.empty(b, 3, H, W)
        r = self.buf("r", b, H, W, 4); self.conv_act("refine_head.1", r1, r[..., :3])
        ops.final_residual(it0, r[..., :3], it_sum, it_final)
        return it_sum, it_final
