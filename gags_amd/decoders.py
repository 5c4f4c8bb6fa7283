"""The per-pixel decoders of the reference, same class names, constructor arguments, parameter
names (`decoder.<i>.weight` / `.bias`: a reference state_dict loads unchanged) and outputs as
models/networks.py:109-218 `CNN_decoder` and :220-248 `CNN_scale_decoder`, computed by hand-written bf16 matrix-core
GEMM kernels (include/gags_next.h N1, csrc/decoder_*.hip) instead of cuDNN 1x1 convolutions.

    CNN_decoder(16, 512):       x [16,H,W] -> 9 x (1x1 conv, 256 hidden, ReLU), x3 = x1 + x2, x5 = x3 + x4 -> F.normalize(dim=0)
    CNN_scale_decoder(16, 3):   x [16,H,W] -> 16-64-128-64-32-16-3 (ReLU between) -> softmax(dim=0)

Input: [C,H,W]; when it is the rasterizer's output (a permuted view of [H,W,C] memory, gaussian_renderer.py) the
pixel-major layout the kernels want is already there and nothing is transposed.  Output: [C_out,H,W] fp32, contiguous.

Precision.  The reference's modules are fp32 Conv2d stacks (models/networks.py:139-218, 220-248; train.py:149,159), and
`precision="exact"` -- the DEFAULT -- computes them with fp32 tensors and fp32-equivalent arithmetic on the 16-bit matrix
cores: every operand as three bfloat16 terms, every product as its six terms of order <= 2, fp32 accumulation
(csrc/decoder_exact.hip); weight gradients are summed over pixel chunks in a fixed order, without atomics
(bit-reproducible).  Against the reference modules' own fp32 results (tests/golden/next_vectors.npz): outputs <= 1e-5,
every gradient <= 1e-3 rel-L2 (tests/test_decoders_gpu.py).
`precision="bf16x2"` (round 4) is the tier matched to what the reference actually computes: torch leaves
`torch.backends.cudnn.allow_tf32` at its default (True) and the reference never touches it, so on the GPU its README names
(RTX 4090, PyTorch 2.1: README.md:26-31) the nn.Conv2d stacks of models/networks.py:145-149,229-233 run in TF32 -- operands
rounded to 10-bit significands.  gfx950 has no TF32; this tier splits every operand into TWO bfloat16 terms (16 significand
bits) and multiplies three matrix terms per product (h h' + h m' + m h'), fp32 tensors and accumulation, the same
deterministic reductions: relative error <= ~2^-16 per product, 32x tighter than TF32, half the matrix work of "exact".
Against the reference modules' own fp32 results: outputs <= 1e-4, every gradient <= 1e-3 (tests/test_decoders_gpu.py).
`precision="f16"` (round 5) is the tier of EQUAL width to the reference's arithmetic: IEEE-half operands carry TF32's own
11-bit significand, products accumulate in fp32 (v_mfma_f32_32x32x16_f16, the rate of the bf16 instruction), activations
and their gradients are stored as half between layers.  It runs the bf16 mode's kernels compiled a second time for the
other operand type (csrc/half16.h: entry points ..._h16), including the fused chains.  What half lacks is exponent range:
conversions saturate at +-65504 instead of producing inf, and the backward multiplies the cotangent by a power of two
chosen on the device from its magnitude (no host sync; `_pow2_scale`) and divides the results by it -- exact, so a
cotangent scaled by 2^k gives gradients scaled by exactly 2^k.  Measured against the reference modules' fp32 autograd:
4.5e-2 worst gradient rel-L2, the same chain with TF32-rounded operands (what the reference's cuDNN convolutions do): 4.6e-2
(tests/test_decoders_gpu.py::test_f16_tier_is_as_close_to_fp32_as_the_tf32_arithmetic_the_reference_runs); one 1080p
iteration 20.4 ms against bf16x2's 62 ms (profiles/r05_d16_iterations.txt).
`precision="bf16"` is the fast opt-in (`dec.precision = "bf16"` or the constructor argument): bf16 operands, fp32
accumulation, activations and their gradients kept in bf16 between layers -- outputs ~5e-3, gradients ~2e-2 of the fp32
results (a low-precision forward flips the ReLU of units within rounding of zero).  Its weight gradients are
deterministic too (partials + ordered sum).  Backward in both modes: input-gradient GEMMs are the forward kernel with
W^T (ReLU mask and skip-connection gradient fused into the epilogue), weight gradients contract over the pixels; the
input gradient comes back in the rasterizer's [H,W,C] layout; gradients nobody asked for (a detached input, frozen
parameters) are not computed.
"""
import ctypes
import weakref

import torch
from torch import nn

from . import _lib
from ._lib import check, ptr

_st = _lib.stream  # (the name the tests call)


# f16 tier: the gradient entering a backward chain is multiplied by a power of two S such that S * max|cotangent proxy| is
# 2^F16_TARGET_LOG2 (half has 5 exponent bits: unscaled, the 1e-9 .. 1e-6 gradients of a mean-reduced loss at 1080p would be
# flushed; conversions saturate at 65504, so a proxy that underestimates costs accuracy on the largest elements, never an inf)
F16_TARGET_LOG2 = 8.0


def _pow2_scale(amax, target_log2=F16_TARGET_LOG2, div=1.0):
    """Device scalars (S, 1 / S), S = 2^floor(target - log2(amax / div)) (1 when amax is 0 or not finite); no host sync, one
    launch (gags_pow2_scale)."""
    a = amax.detach().reshape(1)
    a = a if a.dtype == torch.float32 else a.float()
    out = torch.empty(2, device=a.device)
    check(_lib.load().gags_pow2_scale(ptr(a), float(div), float(target_log2), ptr(out), _lib.stream()), "gags_pow2_scale")
    return out[0:1], out[1:2]


class _SplitTier:
    """An fp32-tensor tier: fp32 weights, activations and gradients, every operand split into `terms` bfloat16 terms
    inside the kernels (3: "exact", 2: "bf16x2"); no fused chain kernels, no gradient scaling."""
    fused, dtype, distill_bwd = False, torch.float32, "gags_decoder_head_distill_bwd_f32"

    def __init__(self, name, terms):
        self.name, self.terms = name, terms

    def weights(self, params):
        # private copies (2.4 MB for CNN_decoder), with the transposes the input-gradient GEMMs contract made NOW: for fp32
        # [co, ci, 1, 1] weights `[:, :, 0, 0].contiguous().float()` is a VIEW of the live parameter, and a backward that runs
        # after an in-place optimizer step would silently differentiate the new weights
        wb = []
        for wt, bs in zip(params[0::2], params[1::2]):
            wm = wt.detach()[:, :, 0, 0].float().clone()
            wm._gags_t = wm.t().contiguous()
            wb.append((wm, bs.detach().float().clone()))
        return wb

    def first_activation(self, p, xp, k):
        return xp

    def layer(self, p, w, b, a1, a2=None, **kw):
        return _xlayer(p, w, b, a1, a2, terms=self.terms, **kw)

    def logits(self, p, w, b, a1, a2=None):
        return _xlayer(p, w, b, a1, a2, relu=False, ldy=_logits_ld(w.shape[0]), terms=self.terms)

    def wgrad(self, p, dz, a1, a2, w, shape, scale):
        dw, db = _xwgrad(p, dz, a1, a2, *w.shape, terms=self.terms)
        return dw.reshape(shape), db

    def cotangent_scale(self, g, div=1.0):
        return None, None

    def head_bwd(self, p, c, head, logits, g, layout):
        dz = torch.empty(p, c, device=g.device)
        check(_lib.load().gags_decoder_head_bwd_exact(p, c, logits.shape[1], head, ptr(logits), ptr(g), layout, ptr(dz), c,
                                                      _lib.stream()), "gags_decoder_head_bwd_exact")
        return dz

    def input_grad(self, gin, h, w, c_in):
        return gin.view(h, w, c_in).permute(2, 0, 1)


class _HalfTier:
    """A 16-bit tier: bf16 operands ("bf16") or IEEE half ("f16": the library's entry points with suffix _h16, csrc/half16.h),
    fp32 accumulation, 16-bit activations and gradients between layers, weights packed once (`_pack_weights`), the fused
    chain kernels.  `scaled`: the backward multiplies the cotangent by a power of two and the results by its inverse."""
    fused = True

    def __init__(self, name, sfx, dtype, scaled):
        self.name, self.sfx, self.dtype, self.scaled = name, sfx, dtype, scaled
        self.distill_bwd = "gags_decoder_head_distill_bwd" + sfx

    def fn(self, base):
        return getattr(_lib.load(), base + self.sfx)

    def weights(self, params):
        return _pack_weights(params[0::2], params[1::2], self)

    def first_activation(self, p, xp, k):
        a0 = torch.empty(p, k, dtype=self.dtype, device=xp.device)
        check(self.fn("gags_decoder_pack_input")(p, xp.shape[1], k, ptr(xp), ptr(a0), _lib.stream()), "gags_decoder_pack_input")
        return a0

    def layer(self, p, w, b, a1, a2=None, **kw):
        return _layer(p, w, b, a1, a2, tier=self, **kw)

    def logits(self, p, w, b, a1, a2=None):
        return _layer(p, w, b, a1, a2, relu=False, f32=True, tier=self)

    def wgrad(self, p, dz, a1, a2, w, shape, scale):
        return _wgrad(p, dz, a1, a2, *w.shape, tier=self, shape=shape, scale=scale)

    def cotangent_scale(self, g, div=1.0):
        if not self.scaled:
            return None, None
        return _pow2_scale(torch.linalg.vector_norm(g.reshape(-1), float("inf")), div=div)  # (max |g| without an |g| temporary)

    def head_bwd(self, p, c, head, logits, g, layout):
        dz = torch.empty(p, logits.shape[1], dtype=self.dtype, device=g.device)
        check(self.fn("gags_decoder_head_bwd")(p, c, logits.shape[1], head, ptr(logits), ptr(g), ptr(dz), layout, _lib.stream()),
              "gags_decoder_head_bwd")
        return dz

    def input_grad(self, gin, h, w, c_in):
        gx = torch.empty(h, w, c_in, device=gin.device)
        check(self.fn("gags_decoder_unpack_grad")(h * w, c_in, gin.shape[1], ptr(gin), ptr(gx), _lib.stream()), "gags_decoder_unpack_grad")
        return gx.permute(2, 0, 1)


_TIERS = {"exact": _SplitTier("exact", 3), "bf16x2": _SplitTier("bf16x2", 2),
          "bf16": _HalfTier("bf16", "", torch.bfloat16, False), "f16": _HalfTier("f16", "_h16", torch.float16, True)}
_BF16, _F16 = _TIERS["bf16"], _TIERS["f16"]  # the 16-bit tiers by the names the bit-identity tests pass to _chain_forward


def _tier(precision):
    if precision not in _TIERS:
        raise ValueError("precision must be 'exact' (fp32-equivalent, the default), 'bf16x2' (two-term split: 16 significand "
                         "bits, tighter than the TF32 the reference's convs run in), 'f16' (IEEE half operands: TF32's own "
                         "11-bit significand, fp32 accumulation, power-of-two gradient scaling) or 'bf16' (8 bits, fast opt-in)")
    return _TIERS[precision]


def _pad32(n):
    return (n + 31) // 32 * 32


def _pixel_major(x):
    """[C,H,W] -> ([P,C] fp32 contiguous, H, W) without a copy when x is a permuted view of [H,W,C] memory."""
    c, h, w = x.shape
    xp = x.permute(1, 2, 0)
    if not (xp.is_contiguous() and xp.dtype == torch.float32):
        xp = xp.contiguous().float()
    return xp.reshape(h * w, c), h, w


def _layer(n_pix, w, b, a1, a2=None, relu=True, f32=False, mask_src=None, residual=None, premask=False, tier=_BF16):
    """One GEMM layer (gags_decoder_layer).  Returns y (16-bit, or fp32 with f32=True) and, with premask=True, also the
    16-bit value before the mask."""
    n, k = w.shape
    dev = w.device
    y = None if f32 else torch.empty(n_pix, n, dtype=tier.dtype, device=dev)
    yf = torch.empty(n_pix, n, device=dev) if f32 else None
    ypre = torch.empty(n_pix, n, dtype=tier.dtype, device=dev) if premask else None
    check(tier.fn("gags_decoder_layer")(n_pix, n, k, ptr(a1), ptr(a2), ptr(w), ptr(b), int(relu), ptr(mask_src),
                                        ptr(residual), ptr(y), ptr(ypre), ptr(yf), _lib.stream()), "gags_decoder_layer")
    out = yf if f32 else y
    return (out, ypre) if premask else out


def _wgrad(n_pix, dz, a1, a2, n, k, tier=_BF16, shape=None, scale=None):
    """Weight and bias gradient of one layer from the padded operands.  shape = the parameter's own (co, ci, ...): the gradient
    is written in that shape (gags_decoder_wgrad_out: no slice copy afterwards); scale: a device scalar every sum is multiplied
    by (the f16 tier's power of two)."""
    co, ci = (n, k) if shape is None else (shape[0], shape[1])
    dw = torch.empty((co, ci) if shape is None else shape, device=dz.device)
    db = torch.empty(co, device=dz.device)
    nb = tier.fn("gags_decoder_wgrad_scratch_bytes")(n_pix, n, k)
    scratch = _lib.scratch(max(nb, 4), dz.device)  # partial matrices per pixel chunk
    check(tier.fn("gags_decoder_wgrad_out")(n_pix, n, k, ptr(dz), ptr(a1), ptr(a2), ptr(dw), ptr(db), co, ci, ptr(scale),
                                            ptr(scratch), nb, _lib.stream()), "gags_decoder_wgrad_out")
    return dw, db


_PACK_CACHE = {}  # (id of the first weight, tier) -> (versions, packed): decoders whose parameters did not change are not repacked


def _pack_weights(weights, biases, tier=_BF16):
    """16-bit [N_pad, K_pad] weights and fp32 [N_pad] biases, every dimension zero-padded to a multiple of 32; each packed
    weight also carries its transpose (for the input-gradient GEMMs) and both in MFMA-fragment order (for the fused
    kernels) as attributes -- one gags_decoder_pack_layers launch for the whole decoder, and none while the parameters' version
    counters stand still (frozen decoders, the second use within one iteration's backward)."""
    key = (id(weights[0]), tier.name)
    vers = tuple((t.data_ptr(), t._version) for t in list(weights) + list(biases))
    hit = _PACK_CACHE.get(key)
    # (the weak references tell a parameter from a later one that got the same id, address and version counter)
    if hit is not None and hit[0] == vers and all(r() is t for r, t in zip(hit[2], list(weights) + list(biases))):
        return hit[1]
    out, srcs, bsrcs, dims = [], [], [], []
    for wt, bs in zip(weights, biases):
        co, ci = wt.shape[:2]
        n, k = _pad32(co), _pad32(ci)
        dev = wt.device
        w = torch.empty(n, k, device=dev, dtype=tier.dtype)
        w_t = torch.empty(k, n, device=dev, dtype=tier.dtype)
        wf = torch.empty(n // 32, k // 16, 2, 32, 8, device=dev, dtype=tier.dtype)
        wtf = torch.empty(k // 32, n // 16, 2, 32, 8, device=dev, dtype=tier.dtype)
        b = torch.empty(n, device=dev)
        src = wt.detach().reshape(co, ci)
        srcs.append(src if (src.is_contiguous() and src.dtype == torch.float32) else src.contiguous().float())
        bsrc = bs.detach()
        bsrcs.append(bsrc if (bsrc.is_contiguous() and bsrc.dtype == torch.float32) else bsrc.contiguous().float())
        dims.append((co, ci))
        w._gags_frag, w._gags_t = wf, w_t
        w_t._gags_frag = wtf
        out.append((w, b))
    for i0 in range(0, len(out), 12):  # one launch per twelve layers (gags_decoder_pack_layers)
        sl = slice(i0, i0 + 12)
        m = len(out[sl])
        ints, ptrs = ctypes.c_int * m, ctypes.c_void_p * m
        check(tier.fn("gags_decoder_pack_layers")(
            m, ints(*[d[0] for d in dims[sl]]), ints(*[d[1] for d in dims[sl]]), ptrs(*[t.data_ptr() for t in srcs[sl]]),
            ptrs(*[t.data_ptr() for t in bsrcs[sl]]), ptrs(*[w.data_ptr() for w, _ in out[sl]]),
            ptrs(*[w._gags_t.data_ptr() for w, _ in out[sl]]), ptrs(*[w._gags_frag.data_ptr() for w, _ in out[sl]]),
            ptrs(*[w._gags_t._gags_frag.data_ptr() for w, _ in out[sl]]), ptrs(*[b.data_ptr() for _, b in out[sl]]), _lib.stream()),
            "gags_decoder_pack_layers")
    if len(_PACK_CACHE) > 16:
        _PACK_CACHE.clear()
    _PACK_CACHE[key] = (vers, out, [weakref.ref(t) for t in list(weights) + list(biases)])
    return out


def invalidate_packed():
    """Forget every packed weight set.  Needed only after a parameter was written through `.data` (which does not move its
    version counter); optimizers, load_state_dict and in-place ops under no_grad all do."""
    _PACK_CACHE.clear()


def _transposed(w):
    """[K_pad, N_pad] of a packed weight (contracts over N in the input-gradient GEMMs)."""
    t = getattr(w, "_gags_t", None)
    return t if t is not None else w.t().contiguous()


def _xlayer(n_pix, w, b, a1, a2=None, relu=True, mask_src=None, residual=None, premask=False, ldy=None, terms=3):
    """One layer on fp32 tensors with every operand split into `terms` bfloat16 terms (gags_decoder_layer_split; 3: exact,
    2: the bf16x2 tier); w [n_out, k_in]; a1 / a2 [n_pix, >= k_in].  ldy > n_out: the extra columns are zero (the head
    kernels want padded logits rows)."""
    n, k = w.shape
    dev = w.device
    ldy = ldy or n
    y = (torch.zeros if ldy > n else torch.empty)(n_pix, ldy, device=dev)
    ypre = torch.empty(n_pix, ldy, device=dev) if premask else None
    check(_lib.load().gags_decoder_layer_split(n_pix, n, k, ptr(a1), ptr(a2), a1.shape[1], ptr(w), ptr(b), int(relu),
                                               ptr(mask_src), ptr(residual), ptr(y), ptr(ypre), ldy, terms, _lib.stream()),
          "gags_decoder_layer_split")
    return (y, ypre) if premask else y


def _xwgrad(n_pix, dz, a1, a2, n, k, want_bias=True, terms=3):
    lib = _lib.load()
    dev = dz.device
    dw = torch.empty(n, k, device=dev)
    db = torch.empty(n, device=dev) if want_bias else None
    nb = lib.gags_decoder_wgrad_exact_scratch_bytes(n_pix, n, k)
    scratch = _lib.scratch(max(nb, 4), dev)
    check(lib.gags_decoder_wgrad_split(n_pix, n, k, ptr(dz), dz.shape[1], ptr(a1), ptr(a2), a1.shape[1], ptr(dw), ptr(db),
                                       ptr(scratch), nb, terms, _lib.stream()), "gags_decoder_wgrad_split")
    return dw, db


def _logits_ld(c_out):
    """Row length of the logits the head kernels read: c_out itself when it is a multiple of 32, else padded to 8."""
    return c_out if c_out % 32 == 0 else (c_out + 7) // 8 * 8


FUSED = True  # 16-bit tiers: a decoder's forward (and input-gradient) chain as one kernel each; False: layer by layer


def _frag_layout(w):
    """bf16 [N, K] (N % 32 == 0, K % 16 == 0) -> [N / 32, K / 16, 64, 8]: the A operand of one v_mfma_f32_32x32x16_bf16 (lane
    32 kh + n holds k = 16 s + 8 kh .. + 7 of row 32 t + n) as one contiguous kilobyte (csrc/decoder_fused.hip: layer_mma)."""
    f = getattr(w, "_gags_frag", None)  # packed by gags_decoder_pack_layer
    if f is not None:
        return f
    n, k = w.shape
    return w.view(n // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()


def _fusable(wb, c_in):
    """The reference's CNN_decoder shape: 9 layers, 256 hidden, c_in <= 32, an output width that is a multiple of 256."""
    shapes = [tuple(w.shape) for w, _ in wb]
    return (len(wb) == 9 and c_in <= 32 and shapes[0] == (256, 32) and all(sh == (256, 256) for sh in shapes[1:8])
            and shapes[8][1] == 256 and shapes[8][0] % 256 == 0)


QUERY_MAX_PHRASES = 32  # positives + negatives of one CNN_decoder.query call (gags_relevancy's cap, csrc/activate.hip)


def _query_phrases(head, device):
    """The phrase operand of gags_decoder_query_fused: [n_pos + n_neg, C] fp32, positives first.  Kept on the head and rebuilt
    when either embedding tensor is another object (RelevancyHead.set_positives) or was written in place (its version
    counter moved), the way _pack_weights follows the parameters.  (The direct head reads the phrases as they are: nothing
    here depends on the decoder's weights.)"""
    pos, neg = head.pos_embeds, head.neg_embeds
    hit = getattr(head, "_gags_query_pack", None)
    if (hit is not None and hit[0] is pos and hit[1] is neg and hit[2] == (pos._version, neg._version)
            and hit[3].device == device):
        return hit[3]
    text = torch.cat([pos.detach().float(), neg.detach().float()]).to(device).contiguous()
    head._gags_query_pack = (pos, neg, (pos._version, neg._version), text)
    return text


_SCALE_SHAPES = [(64, 32), (128, 64), (64, 128), (32, 64), (32, 32), (32, 32)]  # CNN_scale_decoder, padded to 32s


def _scale_fusable(wb, c_in):
    """The reference's CNN_scale_decoder shape (16 -> 64 -> 128 -> 64 -> 32 -> 16 -> 3): csrc/decoder_scale.hip."""
    return c_in <= 32 and [tuple(w.shape) for w, _ in wb] == _SCALE_SHAPES


# The layer wiring of both decoders.  acts[0] is the chain's input and acts[i] the output of layer i - 1; layer i reads
# acts[i], plus acts[j] where _SKIPS[kind] maps i -> j: CNN_decoder's x3 = conv(x1 + x2) and t6 = conv(x3 + x4).
_SKIPS = {"decoder": {3: 1, 6: 4}, "scale": {}}


def _inputs(acts, skips, i):
    """(a1, a2) of layer i, which reads their sum."""
    return (acts[skips[i]], acts[i]) if i in skips else (acts[i], None)


def _fused_forward(tier, kind, p, xp, wb, head_out):
    """The whole chain in one kernel, bit-identical to the layer-by-layer chain: CNN_decoder's nine layers with the
    activations resident in LDS (csrc/decoder_fused.hip), CNN_scale_decoder's six a wave per 32-pixel tile
    (csrc/decoder_scale.hip).  The kernel converts its input tile itself and keeps it as a0; CNN_decoder's keeps x1 + x2 and
    x3 + x4 in place of x2 / x4.  Returns (logits, activations + the ReLU decisions as bits, for the fused backward)."""
    dev = xp.device
    acts = [torch.empty(p, wb[0][0].shape[1], dtype=tier.dtype, device=dev)]
    acts += [torch.empty(p, wgt.shape[0], dtype=tier.dtype, device=dev) for wgt, _ in wb[:-1]]
    arr = ctypes.c_void_p * len(wb)
    wf = [_frag_layout(wgt) for wgt, _ in wb]
    wfs, bs, ats = arr(*[t.data_ptr() for t in wf]), arr(*[b.data_ptr() for _, b in wb]), arr(*[t.data_ptr() for t in acts])
    if kind == "decoder":
        logits = torch.empty(p, wb[-1][0].shape[0], device=dev)
        # 8 layers x whole 64-pixel groups x 8 words (an opaque buffer: the two kernels' own layout)
        masks = torch.empty(8, (p + 63) // 64 * 64, 8, dtype=torch.int32, device=dev)
        check(tier.fn("gags_decoder_fwd_fused")(p, xp.shape[1], logits.shape[1], ptr(xp), wfs, bs, ats, ptr(masks), ptr(logits),
                                                 _lib.stream()), "gags_decoder_fwd_fused")
    else:
        logits = torch.empty(p, 32, device=dev) if head_out is None else None
        masks = torch.empty(p, 11, dtype=torch.int32, device=dev)
        check(tier.fn("gags_scale_decoder_fwd_fused_head")(p, xp.shape[1], ptr(xp), wfs, bs, ats, ptr(masks), ptr(logits),
                                                            ptr(head_out), _lib.stream()), "gags_scale_decoder_fwd_fused_head")
    return logits, acts + [masks]


def _chain_forward(x, kind, params, tier, head_out=None):
    """The GEMM chain of a decoder up to its fp32 logits.  Returns (logits [P, ld], activations, the weights as the tier
    prepared them, h, w, c_in).  head_out (a [3, H, W] fp32 tensor): the fused CNN_scale_decoder kernel writes its softmax
    head there itself and `logits` comes back None (nothing reads them: the head's backward works from its output)."""
    wb = tier.weights(params)
    xp, h, w = _pixel_major(x)
    p, c_in = h * w, xp.shape[1]
    if tier.fused and FUSED and (_fusable if kind == "decoder" else _scale_fusable)(wb, c_in):
        return (*_fused_forward(tier, kind, p, xp, wb, head_out), wb, h, w, c_in)
    skips = _SKIPS[kind]
    acts = [tier.first_activation(p, xp, wb[0][0].shape[1])]
    for i, (wgt, b) in enumerate(wb[:-1]):
        acts.append(tier.layer(p, wgt, b, *_inputs(acts, skips, i)))
    logits = tier.logits(p, *wb[-1], *_inputs(acts, skips, len(wb) - 1))
    return logits, acts, wb, h, w, c_in


def _chain_backward(dz, acts, wb, kind, h, w, c_in, shapes, need_x, need_w, tier, scale=None):
    """From the gradient of the logits dz [P, ld] back through the chain: (input gradient as a [C_in,H,W] view of
    [H,W,C_in] memory, weight / bias gradients in parameter order).  need_x / need_w: what autograd asked for; scale: a
    device scalar every gradient is multiplied by on its way out (the f16 tier's 1 / S)."""
    p = h * w
    wt = [_transposed(wgt) for wgt, _ in wb]  # [K_pad, N_pad]: the input-gradient GEMM contracts over N
    grads = [None] * (2 * len(wb))

    def wg(i, dz_i, a1, a2=None):
        if need_w[i]:  # (written in the parameter's shape, times `scale`: nothing left to do per parameter afterwards)
            grads[2 * i:2 * i + 2] = tier.wgrad(p, dz_i, a1, a2, wb[i][0], shapes[i], scale)

    gx = gin = None
    masks = acts[len(wb)] if len(acts) > len(wb) else None  # the fused forward ran: its ReLU bit masks ride along
    if masks is not None and (kind == "decoder" or (FUSED and dz.shape[1] == 32)):
        # the input-gradient GEMMs in one kernel (bit-identical to the loop below), then the weight gradients; every layer
        # reads the one activation the fused forward kept for it
        dev = dz.device
        dzs = [torch.empty(p, wgt.shape[0], dtype=tier.dtype, device=dev) for wgt, _ in wb[:-1]]
        wtf = [_frag_layout(t) for t in wt]
        arr, arr_dz = ctypes.c_void_p * len(wb), ctypes.c_void_p * len(dzs)
        if kind == "decoder":  # (the kernel also writes the input gradient, times `scale`)
            gx = torch.empty(h, w, c_in, device=dev) if need_x else None
            check(tier.fn("gags_decoder_bwd_fused_scaled")(p, c_in, dz.shape[1], ptr(dz), arr(*[t.data_ptr() for t in wtf]),
                                                           ptr(masks), arr_dz(*[t.data_ptr() for t in dzs]), ptr(gx), ptr(scale),
                                                           _lib.stream()), "gags_decoder_bwd_fused_scaled")
            gx = None if gx is None else gx.permute(2, 0, 1)
        else:
            check(tier.fn("gags_scale_decoder_bwd_fused")(p, ptr(dz), arr(None, *[t.data_ptr() for t in wtf[1:]]), ptr(masks),
                                                          arr_dz(*[t.data_ptr() for t in dzs]), _lib.stream()), "gags_scale_decoder_bwd_fused")
        for i in reversed(range(len(wb))):
            wg(i, dzs[i] if i < len(dzs) else dz, acts[i])
        if kind == "scale" and need_x:
            gin = tier.layer(p, wt[0], None, dzs[0], relu=False)
    else:
        skips, skip_grads = _SKIPS[kind], {}
        cur = dz
        for i in reversed(range(len(wb))):
            wg(i, cur, *_inputs(acts, skips, i))
            if i == 0 and not need_x:
                break
            # W_i^T dz_i, plus what a skip carried back to acts[i], masked by acts[i]'s ReLU; a layer that reads a sum hands
            # the unmasked value on to the skip's source, whose own layer adds it (d(x3 + x4): masked for x4, raw for x3)
            cur = tier.layer(p, wt[i], None, cur, relu=False, mask_src=acts[i] if i > 0 else None,
                             residual=skip_grads.pop(i, None), premask=i in skips)
            if i in skips:
                cur, skip_grads[skips[i]] = cur
        gin = cur if need_x else None
    if gin is not None:
        gx = tier.input_grad(gin, h, w, c_in)
        gx = gx if scale is None else gx * scale
    return gx, grads


def _needs(ctx, first_param):
    """(input gradient wanted, per-layer: weight or bias gradient wanted) from autograd's needs_input_grad."""
    ng = ctx.needs_input_grad
    return bool(ng[0]), [bool(ng[i] or ng[i + 1]) for i in range(first_param, len(ng), 2)]


class _DecoderFn(torch.autograd.Function):
    """Forward and backward of a decoder as GEMM launches.  `kind` = "decoder" (CNN_decoder: two residual sums,
    normalize head) or "scale" (CNN_scale_decoder: plain chain, softmax head).  params = w0, b0, w1, b1, ..."""

    @staticmethod
    def forward(ctx, x, kind, c_out, precision, *params):
        tier = _tier(precision)
        head_out = None
        if tier.fused and kind == "scale" and c_out == 3 and x.dim() == 3:
            head_out = torch.empty(3, x.shape[1], x.shape[2], device=x.device)  # (used when the fused kernel serves the shape)
        logits, acts, wb, h, w, c_in = _chain_forward(x, kind, params, tier, head_out)
        ctx.tier, ctx.kind, ctx.c_out, ctx.hw, ctx.c_in, ctx.wb = tier, kind, c_out, (h, w), c_in, wb
        ctx.shapes = [tuple(t.shape) for t in params[0::2]]
        ctx.from_output = logits is None
        if logits is None:  # the fused scale decoder wrote its softmax head itself; the backward starts from this output
            ctx.save_for_backward(head_out, *acts)
            return head_out
        # CNN_decoder's [C,H,W] output is a permuted view of PIXEL-major memory (like render()'s own output): the head
        # writes rows, the losses read rows, the reference's next step (.permute(1,2,0)) is free.  The 3-channel scale
        # map stays channel-major (its consumers index it by plane).
        p = h * w
        pm = kind == "decoder" and c_out % 4 == 0 and logits.shape[1] <= 512 and logits.shape[1] % 32 == 0
        out = torch.empty((h, w, c_out) if pm else (c_out, h, w), device=x.device)
        check(_lib.load().gags_decoder_head(p, c_out, logits.shape[1], 0 if kind == "decoder" else 1, ptr(logits), ptr(out),
                                            1 if pm else 0, _lib.stream()), "gags_decoder_head")
        if pm:
            out = out.permute(2, 0, 1)
        ctx.save_for_backward(logits, *acts)
        return out

    @staticmethod
    def backward(ctx, g):
        logits, *acts = ctx.saved_tensors
        tier, (h, w), c = ctx.tier, ctx.hw, ctx.c_out
        p = h * w
        gp = g.permute(1, 2, 0)
        pm = (not ctx.from_output and g.dtype == torch.float32 and gp.is_contiguous() and not g.is_contiguous() and c % 4 == 0
              and logits.shape[1] <= 512)  # the cotangent came back in the output's own pixel-major layout
        g = gp if pm else (g if (g.is_contiguous() and g.dtype == torch.float32) else g.contiguous().float())
        s, inv = tier.cotangent_scale(g)  # f16: scaled into half's range by a power of two (exact), the results scaled back
        g = g if s is None else g * s
        if ctx.from_output:  # `logits` is the softmax output y [3, H, W]: dz = y (g - <y, g>) (gags_softmax_head_bwd_y)
            dz = torch.empty(p, 32, dtype=tier.dtype, device=g.device)
            check(tier.fn("gags_softmax_head_bwd_y")(p, c, 32, ptr(logits), ptr(g), ptr(dz), _lib.stream()), "gags_softmax_head_bwd_y")
        else:
            dz = tier.head_bwd(p, c, 0 if ctx.kind == "decoder" else 1, logits, g, 1 if pm else 0)
        need_x, need_w = _needs(ctx, 4)
        gx, grads = _chain_backward(dz, acts, ctx.wb, ctx.kind, h, w, ctx.c_in, ctx.shapes, need_x, need_w, tier, inv)
        return (gx, None, None, None, *grads)


class _DecoderDistillFn(torch.autograd.Function):
    """CNN_decoder + the distillation L1 of train.py:159-166 with the output head fused into the loss: the GEMM chain up
    to the fp32 logits, then ONE kernel to l1_map / mask (gags_decoder_head_distill_fwd) and one back to the logits'
    gradient -- the normalised [512,H,W] map and its gradient are never written or read (21 GB per iteration at 1080p)."""

    @staticmethod
    def forward(ctx, x, img_embed, seg_map, scale_map, c_out, precision, *params):
        from .losses import _f
        tier = _tier(precision)
        logits, acts, wb, h, w, c_in = _chain_forward(x, "decoder", params, tier)
        e, seg, sc = _f(img_embed), _f(seg_map), _f(scale_map)
        if e.shape[1] != c_out or tuple(sc.shape) != (3, h, w) or seg.dim() != 3 or seg.shape[0] != 4:
            raise ValueError(f"embeddings {tuple(e.shape)}, seg_map {tuple(seg.shape)}, scale_map {tuple(sc.shape)} "
                             f"vs a {c_out}-channel {h}x{w} decoder output")
        l1 = torch.empty(h, w, device=x.device)
        mask = torch.empty(h, w, device=x.device)
        check(_lib.load().gags_decoder_head_distill_fwd(c_out, logits.shape[1], h, w, seg.shape[1], seg.shape[2], e.shape[0],
                                                        ptr(logits), ptr(e), ptr(seg), ptr(sc), ptr(l1), ptr(mask), _lib.stream()),
              "gags_decoder_head_distill_fwd")
        ctx.tier, ctx.c_out, ctx.hw, ctx.c_in, ctx.wb = tier, c_out, (h, w), c_in, wb
        ctx.shapes = [tuple(t.shape) for t in params[0::2]]
        ctx.save_for_backward(logits, e, seg, sc, *acts)
        ctx.mark_non_differentiable(mask)
        return l1, mask

    @staticmethod
    def backward(ctx, v_map, _v_mask):
        from .losses import _f
        logits, e, seg, sc, *acts = ctx.saved_tensors
        tier, (h, w), c = ctx.tier, ctx.hw, ctx.c_out
        vm = _f(v_map)
        vs = torch.empty(3, h, w, device=logits.device)
        # the logits' gradient in the tier's type (fp32 in the fp32-tensor tiers).  f16: it is about v_map / (c |logits|),
        # so the kernel multiplies it by a power of two chosen on the device from max |v_map| / c (half has 5 exponent
        # bits), the chain's results are scaled back; the scale map's gradient is fp32
        s, inv = tier.cotangent_scale(vm, div=c)
        dz = torch.empty(h * w, logits.shape[1], dtype=tier.dtype, device=logits.device)
        check(getattr(_lib.load(), tier.distill_bwd)(c, logits.shape[1], h, w, seg.shape[1], seg.shape[2], e.shape[0], ptr(logits),
                                                     ptr(e), ptr(seg), ptr(sc), ptr(vm), ptr(dz), *([] if s is None else [ptr(s)]),
                                                     ptr(vs), _lib.stream()), tier.distill_bwd)
        need_x, need_w = _needs(ctx, 6)
        gx, grads = _chain_backward(dz, acts, ctx.wb, "decoder", h, w, ctx.c_in, ctx.shapes, need_x, need_w, tier, inv)
        return (gx, None, None, vs, None, None, *grads)


class _Stack(nn.Module):
    """A stack of 1x1 convolutions held as nn.Conv2d (+ nn.ReLU entries: the reference's ModuleList indices, so the
    parameter names match) whose forward and backward are run by the GEMM kernels."""
    kind = "scale"

    def __init__(self, dims_in, dims_out, precision="exact"):
        super().__init__()
        _tier(precision)
        self.precision = precision
        layers = []
        for i, (ci, co) in enumerate(zip(dims_in, dims_out)):
            if i > 0:
                layers.append(nn.ReLU())
            layers.append(nn.Conv2d(ci, co, kernel_size=1))
        self.decoder = nn.ModuleList(layers)

    def convs(self):
        return [m for m in self.decoder if isinstance(m, nn.Conv2d)]

    def forward(self, x):
        _lib.on_gpu("decoders", x)
        params = [t for m in self.convs() for t in (m.weight, m.bias)]
        return _DecoderFn.apply(x, self.kind, self.output_dim, self.precision, *params)


class CNN_decoder(_Stack):
    kind = "decoder"

    def __init__(self, input_dim, output_dim, precision="exact"):
        super().__init__([input_dim] + [256] * 8, [256] * 8 + [output_dim], precision)
        self.output_dim = output_dim

    def distill_l1(self, x, img_embed, seg_map, scale_map):
        """train.py:159-166 in one call -- equal to
            feature_map = self(x); gt, mask = read_sam_clip_feature(img_embed, seg_map, scale_map)
            l1_loss_map(feature_map * mask, gt * mask), mask
        with the decoder's normalising head fused into the loss (the [512,H,W] map is never materialised).  Returns
        (l1_map [H,W], mask [1,H,W] bool); gradients reach x, the decoder's parameters and scale_map.  Not part of the
        reference's module: an optional fast path (every precision tier: the fp32-tensor tiers keep the logits' gradient
        in fp32, the bf16 mode rounds it to bf16)."""
        _lib.on_gpu("decoders", x)
        if self.output_dim != 512:
            # other widths: the decoder, then the fused ground-truth assembly + L1 map
            l1, mask = __import__("gags_amd.losses", fromlist=["distill_l1_map"]).distill_l1_map(self(x), img_embed, seg_map, scale_map)
            return l1, mask
        params = [t for m in self.convs() for t in (m.weight, m.bias)]
        l1, mask = _DecoderDistillFn.apply(x, img_embed, seg_map, scale_map, self.output_dim, self.precision, *params)
        return l1, (mask != 0)[None]

    @torch.no_grad()
    def query(self, x, head, pairs=False):
        """The open-vocabulary query of one view (evaluate_iou_loc.py:258-288, compute_relvancy.py:243-269) in one call --
        defined as
            head.get_max_across(self(x).permute(1, 2, 0)[None])[0]          -> [n_pos, H, W] positive probabilities
        or, with pairs=True, head._all(self(x).permute(1, 2, 0).reshape(H * W, -1)) -> [n_pos, H * W, 2] (both entries of the
        winning softmax pair, what get_relevancy returns per phrase).  x: [C_in, H, W] on the GPU; a permuted view of
        pixel-major [H, W, C_in] memory (the rasterizer's output; `f.t()[..., None]` of a per-Gaussian [N, C_in] table) is read
        without a copy.  head: a gags_amd.relevancy.RelevancyHead whose embeddings are `output_dim` wide.  Runs under no_grad.

        In the 16-bit tiers ("bf16", "f16"), for the reference's decoder shape (c_in <= 32, output_dim a multiple of 256) this
        is ONE kernel (csrc/decoder_query.hip, N15): the nine layers per 64-pixel tile in LDS with the bits of the training
        forward, the normalisation and the relevancy of every phrase inside the tile; no activation, logits or normalised map
        is written -- the result is the only allocation.  It equals the composition up to fp32 summation order in the head
        (tests/test_decoder_query_gpu.py: within 4x the composition's own error against float64).  In every other case -- the
        "exact" and "bf16x2" tiers, other shapes, decoders.FUSED = False -- it runs exactly the composition above, and the
        result is bit-identical to what those two calls return.

        Raises ValueError when the head's width is not output_dim, when it has no positive or no negative phrase or more than
        32 phrases in all (gags_relevancy's cap: the composition would fail the same way), RuntimeError on CPU tensors.  (The
        composition has a second limit the kernel does not: gags_relevancy holds its phrases in 60000 bytes of LDS, so 32
        phrases 512 wide run fused and raise in the tiers that compose.)"""
        pos, neg = head.pos_embeds, head.neg_embeds
        if pos.dim() != 2 or neg.dim() != 2 or pos.shape[0] == 0 or neg.shape[0] == 0:
            raise ValueError(f"CNN_decoder.query: the head needs at least one positive and one negative phrase, got "
                             f"{tuple(pos.shape)} and {tuple(neg.shape)}")
        if pos.shape[1] != self.output_dim or neg.shape[1] != self.output_dim:
            raise ValueError(f"CNN_decoder.query: phrase embeddings are {pos.shape[1]} / {neg.shape[1]} wide, the decoder's "
                             f"output {self.output_dim}")
        if pos.shape[0] + neg.shape[0] > QUERY_MAX_PHRASES:
            raise ValueError(f"CNN_decoder.query: {pos.shape[0]} + {neg.shape[0]} phrases, at most {QUERY_MAX_PHRASES} per call")
        if x.dim() != 3:
            raise ValueError(f"CNN_decoder.query: x must be [C_in, H, W], got {tuple(x.shape)}")
        _lib.on_gpu("decoders", x)
        tier = _tier(self.precision)
        if tier.fused and FUSED and self.output_dim % 256 == 0:
            wb = tier.weights([t for m in self.convs() for t in (m.weight, m.bias)])
            xp, h, w = _pixel_major(x)
            if _fusable(wb, xp.shape[1]) and wb[-1][0].shape[0] == self.output_dim:
                text = _query_phrases(head, xp.device)
                arr = ctypes.c_void_p * 9
                probs = torch.empty(pos.shape[0], h * w, 2, device=xp.device)
                check(tier.fn("gags_decoder_query_fused")(h * w, xp.shape[1], self.output_dim, ptr(xp),
                                                          arr(*[_frag_layout(wgt).data_ptr() for wgt, _ in wb]),
                                                          arr(*[b.data_ptr() for _, b in wb]), ptr(text), pos.shape[0], neg.shape[0],
                                                          ptr(probs), _lib.stream()), "gags_decoder_query_fused")
                return probs if pairs else probs[..., 0].reshape(-1, h, w).contiguous()
        feat = self(x).permute(1, 2, 0)
        return head._all(feat.reshape(-1, feat.shape[-1])) if pairs else head.get_max_across(feat[None])[0]


class CNN_scale_decoder(_Stack):
    def __init__(self, input_dim, output_dim, precision="exact"):
        dims = [64, 128, 64, 32, 16, output_dim]
        super().__init__([input_dim] + dims[:-1], dims, precision)
        self.output_dim = output_dim
