"""Thin functional layer over the C ABI: torch tensors in, kernel launches on torch's current HIP stream.

torch is used here for device memory (allocation, views), the current stream and nothing else: every function
below ends in exactly one (or a fixed short sequence of) libwavlm_hip.so entry points.  There is no CPU path --
a CPU tensor raises.
"""
import ctypes as C
import math
import os

import torch

from . import _lib
from ._lib import BF16, F32, ConvRelayoutDesc, GemmDesc, check

_WS = {}


def dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError("unsupported dtype %s (float32 / bfloat16 only)" % t.dtype)


def _dev(t):
    if not t.is_cuda:
        raise _lib.WavlmHipError("unispeech_amd kernels need a HIP device tensor (no CPU fallback)")
    return t.device


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """torch's current HIP stream of the current device as a raw handle (one per launch: the Stream-object route costs
    ~1.5 us of the launch thread per call)"""
    if _RAW_STREAM is not None:
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, offset=0):
    """device address of element `offset` of tensor t (None -> NULL)"""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


WS_MIN_BYTES = 10 << 20   # from here on torch's caching allocator gives a request a segment of its own size


def workspace(device, nbytes, tag="main"):
    """grow-only scratch buffer per (device, tag, stream): reuse is safe because the launches of one stream are ordered.
    At least WS_MIN_BYTES: a long-lived 1 MiB buffer sits in the allocator's small pool and pins a 2 MiB segment whose other half
    stays free for as long as the buffer lives -- a fragment every later small allocation of the process may be handed"""
    key = (device.index, tag, _RAW_STREAM(device.index) if _RAW_STREAM is not None else torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), WS_MIN_BYTES), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _contig(t):
    if t is not None and not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    return t


# --------------------------------------------------------------------------------------------- GEMM
def gemm(A, B, Cc, M, N, K, *, lda, ldb, ldc, transA=False, transB=False, KB=1, sA_kb=0, sB_kb=0, batch=(1, 1),
         sA=(0, 0), sB=(0, 0), sC=(0, 0), a_off=0, b_off=0, c_off=0, alpha=1.0, bias=None, bias_off=0, sBias=(0, 0),
         epi=0, aux=None, aux_off=0, ld_aux=0, sAux=(0, 0), res=None, res_off=0, ld_res=0, sRes=(0, 0),
         accumulate=False, split_k=1, colsum=None, colsum_accumulate=False):
    """C = epi(alpha * sum_kb A.B^T + bias) (+res) (+C); see include/wavlm_hip.h for the addressing rules.
    colsum [N] (optional): (+)= column sums of C over its rows (a bias gradient), fused into the epilogue where possible."""
    dev = _dev(A)
    if A.dtype != B.dtype:
        raise TypeError("A and B must share a dtype")
    d = GemmDesc()
    d.dtype, d.c_dtype = dt(A), dt(Cc)
    d.M, d.N, d.K, d.KB = int(M), int(N), int(K), int(KB)
    d.transA, d.transB = int(bool(transA)), int(bool(transB))
    d.lda, d.ldb, d.ldc = int(lda), int(ldb), int(ldc)
    d.sA_kb, d.sB_kb = int(sA_kb), int(sB_kb)
    d.batch_o, d.batch_i = int(batch[0]), int(batch[1])
    d.sA_o, d.sA_i = int(sA[0]), int(sA[1])
    d.sB_o, d.sB_i = int(sB[0]), int(sB[1])
    d.sC_o, d.sC_i = int(sC[0]), int(sC[1])
    d.A, d.B, d.C = ptr(A, a_off), ptr(B, b_off), ptr(Cc, c_off)
    d.alpha, d.epi = float(alpha), int(epi)
    d.bias = ptr(bias, bias_off)
    d.bias_dtype = dt(bias) if bias is not None else 0
    d.sBias_o, d.sBias_i = int(sBias[0]), int(sBias[1])
    d.aux = ptr(aux, aux_off)
    d.aux_dtype = dt(aux) if aux is not None else 0
    d.ld_aux, d.sAux_o, d.sAux_i = int(ld_aux), int(sAux[0]), int(sAux[1])
    d.res = ptr(res, res_off)
    d.res_dtype = dt(res) if res is not None else 0
    d.ld_res, d.sRes_o, d.sRes_i = int(ld_res), int(sRes[0]), int(sRes[1])
    d.accumulate = int(bool(accumulate))
    d.split_k = int(split_k)
    d.colsum = ptr(colsum)
    d.colsum_dtype = dt(colsum) if colsum is not None else 0
    d.colsum_accumulate = int(bool(colsum_accumulate))
    L = _lib.lib()
    if d.split_k > 1 or colsum is not None:
        need = L.wavlm_gemm_workspace_bytes(C.byref(d))
        ws = workspace(dev, need, "gemm")
        d.workspace, d.ws_bytes = ptr(ws), need
    else:
        d.workspace, d.ws_bytes = None, 0
    check(L.wavlm_gemm(C.byref(d), stream()), "wavlm_gemm[M=%d N=%d K=%d KB=%d tA=%d tB=%d]" % (M, N, K, KB, transA, transB))


def gemm_wgrad_grouped(items, w_dtype):
    """The weight gradients dW_i[N_i, K_i] (+)= dy_i[n, N_i]^T @ x_i[n, K_i] of several linears that share the row count
    n, as ONE grouped split-K launch (wavlm_gemm_grouped) whatever their tiles come to: the kernel checks and the A/B tools.
    items: [(dy2d, x2d, out)] with `out` accumulated into.  (The training path is linear_wgrads.)"""
    dev = _dev(items[0][0])
    n = items[0][0].shape[0]
    tiles = sum(((dy.shape[1] + 255) // 256) * ((x.shape[1] + 255) // 256) for dy, x, _ in items)
    split = grouped_slabs(tiles, (n + 63) // 64)
    L = _lib.lib()
    descs = (GemmDesc * len(items))()
    need = []
    for d, (dy, x, out) in zip(descs, items):
        if dy.shape[0] != n or x.shape[0] != n:
            raise ValueError("grouped weight gradients need a common row count")
        _contig(dy); _contig(x); _contig(out)
        N, K = dy.shape[1], x.shape[1]
        d.dtype, d.c_dtype = dt(dy), dt(out)
        d.M, d.N, d.K, d.KB = N, K, n, 1
        d.transA, d.transB = 1, 1
        d.lda, d.ldb, d.ldc = N, K, K
        d.batch_o, d.batch_i = 1, 1
        d.A, d.B, d.C = ptr(dy), ptr(x), ptr(out)
        d.alpha, d.epi = 1.0, 0
        d.accumulate = 1
        d.split_k = split
        need.append((int(L.wavlm_gemm_workspace_bytes(C.byref(d))) + 255) // 256 * 256)
    ws = workspace(dev, sum(need), "gemm")
    off = 0
    for d, nb in zip(descs, need):
        d.workspace, d.ws_bytes = ptr(ws, off), nb
        off += nb
    check(L.wavlm_gemm_grouped(descs, len(items), stream()), "wavlm_gemm_grouped[%d]" % len(items))


def linear_wgrads(items):
    """dW_i[N_i, K_i] += dy_i[n, N_i]^T @ x_i[n, K_i] for the linears of one block, in arrival order (wavlm_linear_wgrads:
    the library packs them into grouped launches -- the call the fused block makes for its own four).  items: [(dy2d, x2d,
    out)], bf16 operands, every `out` of one dtype and accumulated into."""
    dev = _dev(items[0][0])
    n = items[0][0].shape[0]
    arr = (_lib.WgradItem * len(items))()
    for w, (dy, x, out) in zip(arr, items):
        if dy.shape[0] != n or x.shape[0] != n or dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or out.dtype != items[0][2].dtype:
            raise ValueError("weight gradients of one call share the row count and the dtypes (bf16 operands)")
        _contig(dy); _contig(x); _contig(out)
        w.dy, w.x, w.dW, w.N, w.K = ptr(dy), ptr(x), ptr(out), dy.shape[1], x.shape[1]
    L = _lib.lib()
    need = int(L.wavlm_linear_wgrads_workspace_bytes(arr, len(items), n))
    ws = workspace(dev, need, "gemm")
    check(L.wavlm_linear_wgrads(arr, len(items), n, dt(items[0][2]), ptr(ws), need, stream()), "wavlm_linear_wgrads[%d]" % len(items))


# Launch policy of the weight-gradient GEMMs: the library's (csrc/split_policy.hpp has the rules and their measurements).
# grid = 0, forced = -1, balanced = -1: the process's own settings (CU reservation, WAVLM_WGRAD_SPLIT, lab build with
# WAVLM_WGRAD_STREAMK); explicit values evaluate the same arithmetic.
def grid_blocks():
    """blocks of a persistent GEMM grid: one per CU minus what the data-parallel reducer keeps free (wavlm_set_reserved_cus)"""
    return int(_lib.lib().wavlm_grid_blocks())


def pick_split(M, N, ktiles, grid=0):
    """split-K factor of a single weight-gradient-shaped launch"""
    return int(_lib.lib().wavlm_split_single(M, N, ktiles, grid or 0))


def grouped_split(tiles, ktiles, grid=0, forced=-1):
    """split-K factor of a grouped weight-gradient launch, or 0 when the members should run as single launches"""
    return int(_lib.lib().wavlm_split_grouped(tiles, ktiles, grid or 0, forced))


def grouped_slabs(tiles, ktiles, grid=0, forced=-1, balanced=-1):
    """`split_k` of the members of a grouped weight-gradient launch = fp32 slabs each member's workspace holds"""
    return int(_lib.lib().wavlm_slabs_grouped(tiles, ktiles, grid or 0, forced, int(balanced)))


def wgrad_grouping():
    """False under WAVLM_WGRAD_GROUPING=0: every weight gradient goes out as a single launch"""
    return bool(_lib.lib().wavlm_wgrad_grouping())


# ---------------------------------------------------------------------------------------- row kernels
def layernorm_fwd(x, r, gamma, beta, eps, *, act=0, p_in=0.0, seed_in=0, p_out=0.0, seed_out=0, save=True):
    """returns (y, s, mean, rstd); s is the pre-norm sum (== x when r is None)"""
    dev = _dev(x)
    _contig(x); _contig(r)
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    s = None
    mean = rstd = None
    if save:
        mean = torch.empty(rows, dtype=torch.float32, device=dev)
        rstd = torch.empty(rows, dtype=torch.float32, device=dev)
        s = torch.empty_like(x) if r is not None else x
    check(_lib.lib().wavlm_layernorm_fwd(ptr(x), ptr(r), ptr(y), ptr(s) if (save and r is not None) else None,
                                         ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), rows, D, float(eps), dt(x),
                                         dt(gamma), int(act), float(p_in), int(seed_in), float(p_out), int(seed_out),
                                         stream()), "wavlm_layernorm_fwd")
    return y, s, mean, rstd


# WAVLM_LN_SEG=0: LayerNorm backward never writes the padded conv-gradient layout itself (A/B: the padded copy comes back);
# WAVLM_LN_FULL=0 (the general kernels) has no segmented form either
LN_SEG_OK = os.environ.get("WAVLM_LN_SEG", "1") != "0" and os.environ.get("WAVLM_LN_FULL", "1") != "0"


def layernorm_bwd(dy, s, mean, rstd, gamma, beta, *, act=0, p_in=0.0, seed_in=0, p_out=0.0, seed_out=0,
                  grad_scale=1.0, need_dr=False, dgamma=None, dbeta=None, dr_colsum=None, dx_add=None, dr_incl_add=False,
                  dx_pad=None):
    """returns (dx, dr, dgamma, dbeta, dr_colsum); given dgamma / dbeta (/ dr_colsum) tensors are accumulated into (+=).
    dr_colsum: True -> also return the column sums of dr (fresh tensor); a tensor -> accumulate into it (only together
    with dgamma / dbeta tensors: the three share the accumulate flag).  dx_add: added into dx (not into dr).
    dx_pad = (fp, bp) with dy of shape [B, T, D]: dx is written into a zero-padded [B, fp + T + bp, D] buffer (the layout the
    data-gradient GEMMs of the conv layer in front of this LayerNorm read); returned dx = the [B, T, D] interior VIEW of it,
    whose `_padded` attribute is the whole buffer."""
    dev = _dev(dy)
    _contig(dy); _contig(s)
    if dx_add is not None:
        _contig(dx_add)
        if dx_add.shape != dy.shape or dx_add.dtype != dy.dtype:
            raise ValueError("dx_add must match dy in shape and dtype")
    D = dy.shape[-1]
    rows = dy.numel() // D
    seg_rows = seg_gap = 0
    padded = None
    if dx_pad is not None and (dx_pad[0] or dx_pad[1]):
        fp, bp = dx_pad
        Bn, Tn, _ = dy.shape
        Tp = fp + Tn + bp
        # all pads are the B + 1 equally spaced gaps of one allocation with bp spare rows in front and fp behind (see
        # ConvStackFn.backward): one strided fill
        big = torch.empty((Bn * Tp + fp + bp, D), dtype=dy.dtype, device=dev)
        big.as_strided((Bn + 1, fp + bp, D), (Tp * D, D, 1)).zero_()
        padded = big[bp:bp + Bn * Tp].view(Bn, Tp, D)
        dx = padded[:, fp:fp + Tn]
        seg_rows, seg_gap = Tn, fp + bp
    else:
        dx = torch.empty_like(dy)
    dr = torch.empty_like(dy) if need_dr else None
    acc = dgamma is not None and dbeta is not None
    if not acc:
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(beta)
    if dr_colsum is True or (dr_colsum is not None and not acc):
        if torch.is_tensor(dr_colsum):
            raise ValueError("dr_colsum sink needs dgamma / dbeta sinks")
        dr_colsum = torch.empty_like(gamma) if not acc else torch.zeros_like(gamma)
    L = _lib.lib()
    need = L.wavlm_layernorm_bwd_workspace_bytes(D)
    ws = workspace(dev, need)
    check(L.wavlm_layernorm_bwd_seg(ptr(dy), ptr(s), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dx), ptr(dr),
                                    ptr(dx_add), ptr(dgamma), ptr(dbeta), ptr(dr_colsum), rows, D, dt(dy), dt(gamma), int(act),
                                    float(p_in), int(seed_in), float(p_out), int(seed_out), float(grad_scale), int(acc),
                                    int(bool(dr_incl_add)), seg_rows, seg_gap, ptr(ws), need, stream()), "wavlm_layernorm_bwd_seg")
    if padded is not None:
        dx._padded = padded
    return dx, dr, dgamma, dbeta, dr_colsum


def colsum(x2d, out_dtype, *, include=None, exclude=None, rows=None, N=None, ld=None, out=None, accumulate=False):
    """column sums of a [rows, N] matrix (row stride ld) -> [N] tensor of out_dtype (or (+)= into `out`)"""
    dev = _dev(x2d)
    if rows is None:
        N = x2d.shape[-1]
        rows = x2d.numel() // N
        ld = N
        _contig(x2d)
    if out is None:
        out = torch.empty(N, dtype=out_dtype, device=dev)
        accumulate = False
    L = _lib.lib()
    need = L.wavlm_colsum_workspace_bytes(N)
    ws = workspace(dev, need)
    check(L.wavlm_colsum(ptr(x2d), rows, N, ld, dt(x2d), ptr(include), ptr(exclude), ptr(out), dt(out),
                         int(bool(accumulate)), ptr(ws), need, stream()), "wavlm_colsum")
    return out


def select_rows(x, sel, emb, zero):
    """y[row] = zero[row] ? 0 : sel[row] ? emb : x[row]   (sel / zero: uint8 [rows] or None; emb None -> 0)"""
    _dev(x); _contig(x)
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    check(_lib.lib().wavlm_select_rows(ptr(x), ptr(y), ptr(sel), ptr(emb), ptr(zero), rows, D, dt(x),
                                       dt(emb) if emb is not None else dt(x), stream()), "wavlm_select_rows")
    return y


def gather_rows(src2d, idx, n_out):
    """dst[i] = src[idx[i]] (idx int32; -1 -> zero row)"""
    dev = _dev(src2d); _contig(src2d)
    D = src2d.shape[-1]
    dst = torch.empty((n_out, D), dtype=src2d.dtype, device=dev)
    check(_lib.lib().wavlm_gather_rows(ptr(src2d), ptr(idx), ptr(dst), n_out, D, dt(src2d), stream()),
          "wavlm_gather_rows")
    return dst


def _conv_desc(weights, specs):
    d = ConvRelayoutDesc()
    if len(weights) > 8:
        raise ValueError("at most 8 convolution layers per call")
    d.n_layers, d.dtype = len(weights), dt(weights[0])
    for l, (W, (k, s_)) in enumerate(zip(weights, specs)):
        _dev(W); _contig(W)
        Cout, Cin, kk = W.shape
        if kk != k:
            raise ValueError("kernel width of layer %d does not match its spec" % l)
        d.Cout[l], d.Cin[l], d.k[l], d.s[l] = Cout, Cin, k, s_
        d.W[l] = W.data_ptr()
    return d


def conv_weights_relayout(weights, specs, want_bwd):
    """GEMM operand images of the extractor's Conv1d weights, all layers in one launch.  weights: [Cout, Cin, k] tensors,
    specs: [(k, stride)].  Returns (Wf list [Cout, k * Cin], Wb flat buffers [Cin * Cout * k] or None): the stride-phase
    images of layer l are views of its flat buffer (conv_phase_views)."""
    d = _conv_desc(weights, specs)
    Wf, Wb = [], []
    for l, (W, (k, s_)) in enumerate(zip(weights, specs)):
        Cout, Cin, _ = W.shape
        f = torch.empty((Cout, k * Cin), dtype=W.dtype, device=W.device)
        d.Wf[l] = f.data_ptr()
        Wf.append(f)
        if want_bwd:
            flat = torch.empty(Cin * Cout * k, dtype=W.dtype, device=W.device)
            d.Wb[l] = flat.data_ptr()
            Wb.append(flat)
        else:
            d.Wb[l] = None
    check(_lib.lib().wavlm_conv_weights_relayout(C.byref(d), stream()), "wavlm_conv_weights_relayout")
    return Wf, (Wb if want_bwd else None)


def conv_phase_views(flat, Cout, Cin, k, s_):
    """the s_ stride-phase images [Cin, J_r * Cout] (taps of phase r newest first) inside a layer's flat Wb buffer"""
    views, off = [], 0
    for r in range(s_):
        Jr = len(range(r, k, s_))
        views.append(flat[off:off + Cin * Jr * Cout].view(Cin, Jr * Cout))
        off += Cin * Jr * Cout
    return views


def conv_wgrad_scatter(grads, dWf, specs, accumulate):
    """grads[l][co][ci][kk] (+)= dWf[l][co][kk * Cin + ci] for all layers in one launch"""
    d = _conv_desc(grads, specs)
    for l, f in enumerate(dWf):
        _contig(f)
        d.Wf[l] = f.data_ptr()
        d.Wb[l] = None
    check(_lib.lib().wavlm_conv_wgrad_scatter(C.byref(d), int(bool(accumulate)), stream()), "wavlm_conv_wgrad_scatter")


def axpby_(y, x, a, b):
    """y = a*x + b*y in place"""
    _dev(y); _contig(y); _contig(x)
    check(_lib.lib().wavlm_axpby(ptr(x), dt(x), ptr(y), dt(y), y.numel(), float(a), float(b), stream()), "wavlm_axpby")
    return y


def scale_dev_(y, scalar, extra=1.0):
    """y *= scalar[0] * extra with `scalar` a 1-element fp32 device tensor"""
    _dev(y); _contig(y)
    check(_lib.lib().wavlm_scale_dev(ptr(y), dt(y), y.numel(), ptr(scalar), float(extra), stream()), "wavlm_scale_dev")
    return y


def dropout(x, p, seed):
    _dev(x); _contig(x)
    y = torch.empty_like(x)
    check(_lib.lib().wavlm_dropout(ptr(x), ptr(y), x.numel(), float(p), int(seed), dt(x), stream()), "wavlm_dropout")
    return y


def dropout_add(x, r, p, seed):
    """x + dropout(r, p, seed) in one pass (p = 0: plain add)"""
    _dev(x); _contig(x); _contig(r)
    y = torch.empty_like(x)
    check(_lib.lib().wavlm_dropout_add(ptr(x), ptr(r), ptr(y), x.numel(), float(p), int(seed), dt(x), stream()),
          "wavlm_dropout_add")
    return y


def _replace_mix_args(t, sel):
    _dev(t); _contig(t); _contig(sel)
    D = t.shape[-1]
    rows = t.numel() // D if D else 0
    if sel.dtype != torch.uint8 or sel.numel() != rows or sel.device != t.device:
        raise ValueError("sel: expected uint8 [rows = %d] on the tensors' device" % rows)
    return rows, D


def replace_mix(x, q, sel, p, seed):
    """y[row] = dropout(sel[row] ? q[row] : x[row], p, seed) over the rows of [..., D] tensors (sel uint8, one per row); the keep
    decisions are those of dropout() for the same seed"""
    rows, D = _replace_mix_args(x, sel)
    _contig(q)
    if q.shape != x.shape or q.dtype != x.dtype or q.device != x.device:
        raise ValueError("x and q must share shape, dtype and device")
    y = torch.empty_like(x)
    if rows == 0:     # (an empty tensor has no address to hand over)
        return y
    check(_lib.lib().wavlm_replace_mix(ptr(x), ptr(q), ptr(sel), ptr(y), rows, D, float(p), int(seed), dt(x), stream()),
          "wavlm_replace_mix")
    return y


def replace_mix_bwd(g, sel, p, seed):
    """(dx, dq) of replace_mix for the incoming gradient g"""
    rows, D = _replace_mix_args(g, sel)
    dx, dq = torch.empty_like(g), torch.empty_like(g)
    if rows == 0:
        return dx, dq
    check(_lib.lib().wavlm_replace_mix_bwd(ptr(g), ptr(sel), ptr(dx), ptr(dq), rows, D, float(p), int(seed), dt(g), stream()),
          "wavlm_replace_mix_bwd")
    return dx, dq


def sumsq(x, scale=1.0, out=None):
    """scale * sum(x^2) as a 1-element fp32 device tensor (no host sync)"""
    dev = _dev(x); _contig(x)
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=dev)
    L = _lib.lib()
    need = L.wavlm_sumsq_workspace_bytes()
    ws = workspace(dev, need, "reduce")
    check(L.wavlm_sumsq(ptr(x), dt(x), x.numel(), float(scale), ptr(out), ptr(ws), need, stream()), "wavlm_sumsq")
    return out


def sum_f32(x, out=None):
    dev = _dev(x); _contig(x)
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=dev)
    L = _lib.lib()
    need = L.wavlm_sum_workspace_bytes()
    ws = workspace(dev, need, "reduce")
    check(L.wavlm_sum_f32(ptr(x), x.numel(), ptr(out), ptr(ws), need, stream()), "wavlm_sum_f32")
    return out


# -------------------------------------------------------------------------------------------- conv0
def conv0_gn_gelu_fwd(wav, W, gamma, beta, stride, eps, out_dtype):
    dev = _dev(wav); _contig(wav); _contig(W)
    B, T = wav.shape
    Cc, _, kw = W.shape
    T0 = (T - kw) // stride + 1
    out = torch.empty((B, T0, Cc), dtype=out_dtype, device=dev)
    stats = torch.empty((B, Cc, 2), dtype=torch.float32, device=dev)
    L = _lib.lib()
    need = L.wavlm_conv0_gn_workspace_bytes(B, T, Cc, stride)
    ws = workspace(dev, need)
    check(L.wavlm_conv0_gn_gelu_fwd(ptr(wav), dt(wav), ptr(W), ptr(gamma), ptr(beta), dt(W), ptr(out), dt(out),
                                    ptr(stats), B, T, Cc, kw, stride, float(eps), ptr(ws), need, stream()),
          "wavlm_conv0_gn_gelu_fwd")
    return out, stats


def conv0_gn_gelu_bwd(wav, W, gamma, beta, g, stats, stride, gscale=1.0):
    dev = _dev(wav); _contig(g)
    B, T = wav.shape
    Cc, _, kw = W.shape
    dW = torch.empty_like(W)
    dgamma = torch.empty_like(gamma)
    dbeta = torch.empty_like(beta)
    L = _lib.lib()
    need = L.wavlm_conv0_gn_bwd_workspace_bytes(B, T, Cc, stride)
    ws = workspace(dev, need)
    check(L.wavlm_conv0_gn_gelu_bwd(ptr(wav), dt(wav), ptr(W), ptr(gamma), ptr(beta), dt(W), ptr(g), dt(g),
                                    ptr(stats), ptr(dW), ptr(dgamma), ptr(dbeta), B, T, Cc, kw, stride,
                                    float(gscale), ptr(ws), need, stream()), "wavlm_conv0_gn_gelu_bwd")
    return dW, dgamma, dbeta


def conv0_ln_gelu_fwd(wav, W, gamma, beta, stride, eps, out_dtype, bias=None):
    """extractor_mode 'layer_norm', block 0: gelu(LayerNorm_C(conv0(wav) + bias)) -> [B, T0, C]"""
    dev = _dev(wav); _contig(wav); _contig(W)
    B, T = wav.shape
    Cc, _, kw = W.shape
    T0 = (T - kw) // stride + 1
    out = torch.empty((B, T0, Cc), dtype=out_dtype, device=dev)
    L = _lib.lib()
    need = L.wavlm_conv0_ln_fwd_workspace_bytes()
    ws = workspace(dev, need)
    check(L.wavlm_conv0_ln_gelu_fwd(ptr(wav), dt(wav), ptr(W), ptr(bias), ptr(gamma), ptr(beta), dt(W), ptr(out), dt(out), B, T,
                                    Cc, kw, stride, float(eps), ptr(ws), need, stream()), "wavlm_conv0_ln_gelu_fwd")
    return out


def conv0_ln_gelu_bwd(wav, W, gamma, beta, g, stride, eps, gscale=1.0, bias=None):
    """returns (dW, dgamma, dbeta, dbias); dbias is None without a conv bias"""
    dev = _dev(wav); _contig(g)
    B, T = wav.shape
    Cc, _, kw = W.shape
    dW = torch.empty_like(W)
    dgamma = torch.empty_like(gamma)
    dbeta = torch.empty_like(beta)
    dbias = torch.empty_like(bias) if bias is not None else None
    L = _lib.lib()
    need = L.wavlm_conv0_ln_bwd_workspace_bytes(B, T, Cc, stride)
    ws = workspace(dev, need)
    check(L.wavlm_conv0_ln_gelu_bwd(ptr(wav), dt(wav), ptr(W), ptr(bias), ptr(gamma), ptr(beta), dt(W), ptr(g), dt(g),
                                    ptr(dW), ptr(dbias), ptr(dgamma), ptr(dbeta), B, T, Cc, kw, stride, float(eps),
                                    float(gscale), ptr(ws), need, stream()), "wavlm_conv0_ln_gelu_bwd")
    return dW, dgamma, dbeta, dbias


# ---------------------------------------------------------------------------------------- attention
def relpos_gather(emb, bucket, H, L_):
    dev = _dev(emb)
    tab = torch.empty((H, L_), dtype=torch.float32, device=dev)
    check(_lib.lib().wavlm_relpos_gather(ptr(emb), dt(emb), ptr(bucket), ptr(tab), H, L_, stream()),
          "wavlm_relpos_gather")
    return tab


def relpos_scatter(dtab, bucket, like_emb):
    H, L_ = dtab.shape
    demb = torch.empty_like(like_emb)
    check(_lib.lib().wavlm_relpos_scatter(ptr(dtab), ptr(bucket), ptr(demb), dt(demb), H, L_, like_emb.shape[0],
                                          stream()), "wavlm_relpos_scatter")
    return demb


def gate_fwd(x, W, bias, grep_a, H):
    dev = _dev(x); _contig(x)
    B, T, D = x.shape
    hd = D // H
    gate = torch.empty((B, H, T), dtype=torch.float32, device=dev)
    ga = torch.empty_like(gate)
    gb = torch.empty_like(gate)
    check(_lib.lib().wavlm_gate_fwd(ptr(x), ptr(W), ptr(bias), ptr(grep_a), ptr(gate), ptr(ga), ptr(gb), B, T, H, hd,
                                    dt(x), dt(W), stream()), "wavlm_gate_fwd")
    return gate, ga, gb


def gate_bwd(dgate, x, W, bias, grep_a, ga, gb, H, sinks=None, dx_accumulate=None):
    """returns (dx, dW, dbias, da); sinks = (dW, dbias, da) gradient-sink views -> accumulated in place, returned as None;
    dx_accumulate: a [B, T, D] tensor already holding another consumer's gradient of x -> the gate's is added into it"""
    dev = _dev(x)
    B, T, D = x.shape
    hd = D // H
    dx = dx_accumulate if dx_accumulate is not None else torch.empty_like(x)
    _contig(dx)
    if sinks is not None:
        dW, dbias, da = sinks
    else:
        dW = torch.empty_like(W)
        dbias = torch.empty_like(bias)
        da = torch.empty_like(grep_a)
    L = _lib.lib()
    need = L.wavlm_gate_bwd_workspace_bytes(H, hd)
    ws = workspace(dev, need)
    check(L.wavlm_gate_bwd(ptr(dgate), ptr(x), ptr(W), ptr(grep_a), ptr(ga), ptr(gb), ptr(dx), ptr(dW), ptr(dbias),
                           ptr(da), B, T, H, hd, dt(x), dt(W), int(sinks is not None) | (2 if dx_accumulate is not None else 0),
                           ptr(ws), need, stream()),
          "wavlm_gate_bwd")
    if sinks is not None:
        return dx, None, None, None
    return dx, dW, dbias, da


def attn_softmax_fwd(S, P, lse, gate, tab, kpm, B, H, T, ldS, ldP, p_drop, seed):
    check(_lib.lib().wavlm_attn_softmax_fwd(ptr(S), ptr(P), ptr(lse), ptr(gate), ptr(tab), ptr(kpm), B, H, T, ldS, ldP,
                                            dt(S), dt(P), float(p_drop), int(seed), stream()),
          "wavlm_attn_softmax_fwd")


def attn_softmax_bwd(S, dP, lse, gate, tab, kpm, dS, dgate, dtab, B, H, T, ldS, ldP, p_drop, seed):
    dev = _dev(S)
    L = _lib.lib()
    need = L.wavlm_attn_softmax_bwd_workspace_bytes(B, H, T) if tab is not None else 0
    ws = workspace(dev, need) if need else None
    check(L.wavlm_attn_softmax_bwd(ptr(S), ptr(dP), ptr(lse), ptr(gate), ptr(tab), ptr(kpm), ptr(dS), ptr(dgate),
                                   ptr(dtab), 0, B, H, T, ldS, ldP, dt(S), dt(dS), float(p_drop), int(seed), ptr(ws),
                                   need, stream()), "wavlm_attn_softmax_bwd")


def attn_fused_fwd(qkv, gate, tab, kpm, H, scale, p_drop, seed, store_p=False):
    """fused bf16 attention forward (head_dim 64): returns (O [B,T,D], lse [B*H,T], pstore).  store_p True: the forward also
    writes its probabilities into `pstore` (opaque uint8 buffer) for attn_fused_bwd; "bits": only its dropout decisions (one
    bit per element; nothing without dropout); False: pstore is None"""
    dev = _dev(qkv); _contig(qkv)
    B, T, D3 = qkv.shape
    D = D3 // 3
    O = torch.empty((B, T, D), dtype=qkv.dtype, device=dev)
    lse = torch.empty((B * H, T), dtype=torch.float32, device=dev)
    L = _lib.lib()
    pstore, nps = None, 0
    if store_p == "bits":
        if p_drop > 0:
            nps = int(L.wavlm_attn_fused_dbits_bytes(B, H, T))
            pstore = torch.empty(nps, dtype=torch.uint8, device=dev)
    elif store_p:
        nps = int(L.wavlm_attn_fused_pstore_bytes(B, H, T))   # 0: this T is not supported by the stored form -> recompute
        pstore = torch.empty(nps, dtype=torch.uint8, device=dev) if nps else None
    check(L.wavlm_attn_fused_fwd_p(ptr(qkv), ptr(O), ptr(lse), ptr(gate), ptr(tab), ptr(kpm), ptr(pstore), nps, B, H, T, D // H,
                                   float(scale), float(p_drop), int(seed), stream()), "wavlm_attn_fused_fwd_p")
    return O, lse, pstore


def attn_fused_bwd(qkv, O, dO, lse, gate, tab, kpm, H, scale, p_drop, seed, dbias=None, dbias_accumulate=False, pstore=None):
    """returns (dqkv, dgate, dtab); dbias [3D] (optional, any float dtype): (+)= column sums of dqkv (q|k|v bias gradient);
    pstore: what attn_fused_fwd(store_p=True) returned for the same arguments (None: probabilities are recomputed)"""
    dev = _dev(qkv); _contig(dO)
    B, T, D3 = qkv.shape
    D = D3 // 3
    dqkv = torch.empty_like(qkv)
    dgate = dtab = None
    if tab is not None:
        dgate = torch.empty((B, H, T), dtype=torch.float32, device=dev)
        dtab = torch.empty_like(tab)
    L = _lib.lib()
    need = L.wavlm_attn_fused_bwd_workspace_bytes(B, H, T)
    ws = workspace(dev, need, "attn")
    check(L.wavlm_attn_fused_bwd_p(ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(gate), ptr(tab), ptr(kpm), ptr(pstore),
                                   pstore.numel() if pstore is not None else 0, ptr(dqkv),
                                   ptr(dgate), ptr(dtab), ptr(dbias), dt(dbias) if dbias is not None else 0,
                                   int(bool(dbias_accumulate)), B, H, T, D // H, float(scale), float(p_drop), int(seed),
                                   ptr(ws), need, stream()), "wavlm_attn_fused_bwd_p")
    return dqkv, dgate, dtab


# ------------------------------------------------------------------------------------------ pos_conv
def posconv_weight_fwd(v, g, out_dtype, layout=0):
    """layout 0: operand images of the GEMM form; 1: of the direct convolution (posconv_direct)"""
    dev = _dev(v); _contig(v)
    D, Cg, K = v.shape
    G = D // Cg
    Wf = torch.empty((G, Cg, K * Cg), dtype=out_dtype, device=dev)
    Wb = torch.empty((G, Cg, K * Cg), dtype=out_dtype, device=dev)
    norm = torch.empty(K, dtype=torch.float32, device=dev)
    L = _lib.lib()
    need = L.wavlm_posconv_weight_workspace_bytes(D, Cg, K)
    ws = workspace(dev, need)
    check(L.wavlm_posconv_weight_fwd(ptr(v), ptr(g), dt(v), ptr(Wf), ptr(Wb), dt(Wf), ptr(norm), D, Cg, K, int(layout),
                                     ptr(ws), need, stream()), "wavlm_posconv_weight_fwd")
    return Wf, Wb, norm


def posconv_weight_bwd(dWf, v, g, norm, nsplit=1):
    """dWf: fp32 [nsplit, G, Cg, K*Cg] (slabs are summed)"""
    dev = _dev(v)
    D, Cg, K = v.shape
    dv = torch.empty_like(v)
    dg = torch.empty_like(g)
    L = _lib.lib()
    need = L.wavlm_posconv_weight_workspace_bytes(D, Cg, K)
    ws = workspace(dev, need)
    check(L.wavlm_posconv_weight_bwd(ptr(dWf), ptr(v), ptr(g), ptr(norm), dt(v), ptr(dv), ptr(dg), D, Cg, K, int(nsplit),
                                     ptr(ws), need, stream()), "wavlm_posconv_weight_bwd")
    return dv, dg


def group_major(x, aux, G, left_pad, Tp, want_nat=False, aux_is_grad=False):
    """x[B,T,D] (* gelu'(aux), or * aux if it already holds the derivative) -> [B,G,Tp,D/G], zero rows outside
    [left_pad, left_pad+T)"""
    dev = _dev(x); _contig(x); _contig(aux)
    B, T, D = x.shape
    out = torch.empty((B, G, Tp, D // G), dtype=x.dtype, device=dev)
    nat = torch.empty_like(x) if want_nat else None
    check(_lib.lib().wavlm_posconv_group_major(ptr(x), ptr(aux), ptr(out), ptr(nat), B, T, D, G, left_pad, Tp, dt(x),
                                               int(bool(aux_is_grad)), stream()), "wavlm_posconv_group_major")
    return out, nat


def posconv_dw_direct(xg, dug, du_off, T, K):
    """weight gradient of the grouped convolution from the two group-major copies -> (fp32 slabs [S, G, Cg, K*Cg], S)"""
    dev = _dev(xg); _contig(xg); _contig(dug)
    B, G, Tp, Cg = xg.shape
    L = _lib.lib()
    S = L.wavlm_posconv_dw_direct_splits(Cg, G)
    if S <= 0:
        raise ValueError("posconv_dw_direct: shape not covered")
    part = torch.empty((S, G, Cg, K * Cg), dtype=torch.float32, device=dev)
    check(L.wavlm_posconv_dw_direct(ptr(xg), ptr(dug), ptr(part), B, G, T, Tp, int(du_off), Cg, K, stream()),
          "wavlm_posconv_dw_direct")
    return part, S


def posconv_direct_supported(x_dtype, Cg, K, T):
    return x_dtype == torch.bfloat16 and bool(_lib.lib().wavlm_posconv_direct_supported(int(Cg), int(K), int(T)))


def posconv_direct(xg, W, out, T, K, *, bias=None, res=None, aux=None, gelu=False):
    """grouped convolution over the group-major, time-padded copy xg [B, G, Tp, Cg] with the weight image W [G, Cg, K*Cg]:
    out[B, T, G*Cg] = res + f(conv + bias), f = GELU (aux receives the pre-activation) or identity"""
    _dev(xg); _contig(xg); _contig(W); _contig(out); _contig(res); _contig(aux)
    B, G, Tp, Cg = xg.shape
    check(_lib.lib().wavlm_posconv_direct(ptr(xg), ptr(W), ptr(bias), ptr(res), ptr(out), ptr(aux), B, G, T, Tp, Cg, K,
                                          int(bool(gelu)), stream()), "wavlm_posconv_direct")
    return out


# ---------------------------------------------------------------------------------------------- loss
def l2norm_fwd(x, out_dtype, eps=1e-8):
    dev = _dev(x); _contig(x)
    rows, D = x.shape
    y = torch.empty((rows, D), dtype=out_dtype, device=dev)
    inv = torch.empty(rows, dtype=torch.float32, device=dev)
    check(_lib.lib().wavlm_l2norm_fwd(ptr(x), dt(x), ptr(y), dt(y), ptr(inv), rows, D, float(eps), stream()),
          "wavlm_l2norm_fwd")
    return y, inv


def l2norm_bwd(dy, y, inv, x_dtype):
    dev = _dev(dy); _contig(dy)
    rows, D = y.shape
    dx = torch.empty((rows, D), dtype=x_dtype, device=dev)
    check(_lib.lib().wavlm_l2norm_bwd(ptr(dy), ptr(y), dt(y), ptr(inv), ptr(dx), dt(dx), rows, D, stream()),
          "wavlm_l2norm_bwd")
    return dx


def ce_rows(logits, target, V, ld_logits, dlogits, ld_dlogits, weight, flat_wrong=False):
    """flat_wrong: a row whose V logits are all equal is not correct (the wav2vec criterion's arg-min rule)"""
    dev = _dev(logits)
    S = target.numel()
    loss_rows = torch.empty(max(S, 1), dtype=torch.float32, device=dev)
    correct_rows = torch.empty(max(S, 1), dtype=torch.float32, device=dev)
    check(_lib.lib().wavlm_ce_rows(ptr(logits), ptr(target), ptr(loss_rows), ptr(correct_rows), ptr(dlogits),
                                   dt(dlogits) if dlogits is not None else 0, S, V, ld_logits, ld_dlogits,
                                   float(weight), int(bool(flat_wrong)), stream()), "wavlm_ce_rows")
    return loss_rows[:S], correct_rows[:S]


# --------------------------------------------------------------------------------------------- optim
def adam_step(p32, m, v, grad, p_lowp, *, lr, beta1, beta2, eps, weight_decay, step, grad_mult=1.0,
              grad_mult_dev=None, gnorm_sq=None, max_norm=0.0):
    _dev(p32)
    check(_lib.lib().wavlm_adam_step(ptr(p32), ptr(m), ptr(v), ptr(grad), dt(grad), ptr(p_lowp),
                                     dt(p_lowp) if p_lowp is not None else 0, p32.numel(), float(lr), float(beta1),
                                     float(beta2), float(eps), float(weight_decay), int(step), float(grad_mult),
                                     ptr(grad_mult_dev), ptr(gnorm_sq), float(max_norm), stream()), "wavlm_adam_step")


def gemm_set_variant(v):
    """0 auto | 1 force the 128x128 tile | 2 force the 256x128 tile (tests / A-B measurements)"""
    _lib.lib().wavlm_gemm_set_variant(int(v))


def set_reserved_cus(n):
    """leave n CUs out of every persistent GEMM grid (data-parallel runs: room for the RCCL kernels)"""
    _lib.lib().wavlm_set_reserved_cus(int(n))


def get_reserved_cus():
    return int(_lib.lib().wavlm_get_reserved_cus())


def prof_enable(on):
    _lib.lib().wavlm_prof_enable(1 if on else 0)


def prof_collect(dtype=-1):
    """(launches, total_ms, total_flops) of the GEMM launches recorded since prof_enable(True); synchronises"""
    ms, fl = C.c_double(0.0), C.c_double(0.0)
    n = _lib.lib().wavlm_prof_collect(int(dtype), C.byref(ms), C.byref(fl))
    return n, ms.value, fl.value


PROF_CLASSES = {"gemm": 0, "attn_fwd": 1, "attn_bwd": 2, "conv0_fwd": 3, "conv0_bwd": 4, "ln_fwd": 5, "ln_bwd": 6}


def prof_collect_class(name):
    """(calls, total_ms, algorithmic flops, algorithmic bytes) of one kernel class (PROF_CLASSES) recorded since
    prof_enable(True); synchronises"""
    ms, fl, by = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    n = _lib.lib().wavlm_prof_collect_class(PROF_CLASSES[name], C.byref(ms), C.byref(fl), C.byref(by))
    return n, ms.value, fl.value, by.value


def prof_collect_bytes(dtype=-1):
    """algorithmic HBM bytes (each operand / output / epilogue tensor once) of the launches prof_collect reports"""
    return float(_lib.lib().wavlm_prof_collect_bytes(int(dtype)))


# ------------------------------------------------------------------------- sampled-instance cosine head
GLU_GATES = {"sigmoid": 0, "swish": 1, "relu": 2, "gelu": 3, "bilinear": 4}
ACT_KINDS = {"relu": 1, "gelu_accurate": 2, "gelu_fast": 2, "tanh": 3, "gelu": 4}


def glu_fwd(x2d, gate="sigmoid"):
    """[rows, 2F] -> [rows, F]: x[:, :F] * g(x[:, F:]); gate "sigmoid" = nn.GLU(dim=-1), "swish" = GLU_Linear's"""
    _dev(x2d); _contig(x2d)
    rows, F2 = x2d.shape
    y = torch.empty((rows, F2 // 2), dtype=x2d.dtype, device=x2d.device)
    check(_lib.lib().wavlm_glu_fwd(ptr(x2d), ptr(y), rows, F2 // 2, dt(x2d), GLU_GATES[gate], stream()), "wavlm_glu_fwd")
    return y


def glu_bwd(x2d, dy, gate="sigmoid"):
    _dev(x2d); _contig(x2d); _contig(dy)
    rows, F2 = x2d.shape
    dx = torch.empty_like(x2d)
    check(_lib.lib().wavlm_glu_bwd(ptr(x2d), ptr(dy), ptr(dx), rows, F2 // 2, dt(x2d), GLU_GATES[gate], stream()), "wavlm_glu_bwd")
    return dx


def act_fwd(x, kind):
    """elementwise activation (ACT_KINDS) of a contiguous tensor"""
    _dev(x); _contig(x)
    y = torch.empty_like(x)
    check(_lib.lib().wavlm_act_fwd(ptr(x), ptr(y), x.numel(), dt(x), ACT_KINDS[kind], stream()), "wavlm_act_fwd")
    return y


def act_bwd(x, dy, kind):
    """dx = dy * act'(x), x the pre-activation"""
    _dev(x); _contig(x); _contig(dy)
    dx = torch.empty_like(x)
    check(_lib.lib().wavlm_act_bwd(ptr(x), ptr(dy), ptr(dx), x.numel(), dt(x), ACT_KINDS[kind], stream()), "wavlm_act_bwd")
    return dx


def gather_dot(X, Y, idx, scale, mask_raw=None):
    """out[s, n] = scale * <X[s], Y[idx[s, n]]>  (rows [., D], idx: int32 [S, N]); mask_raw: the rows of Y before
    normalisation -- columns n >= 1 whose gathered row of mask_raw equals the row of column 0 become -inf"""
    dev = _dev(Y); _contig(X); _contig(Y); _contig(idx); _contig(mask_raw)
    if mask_raw is not None and (mask_raw.shape != Y.shape or mask_raw.dtype != Y.dtype):
        raise ValueError("gather_dot: mask_raw must have the shape and dtype of Y")
    S, N = idx.shape
    out = torch.empty((S, N), dtype=torch.float32, device=dev)
    check(_lib.lib().wavlm_gather_dot(ptr(X), ptr(Y), dt(Y), ptr(idx), ptr(out), S, N, Y.shape[1], float(scale),
                                      ptr(mask_raw), stream()), "wavlm_gather_dot")
    return out


def rows_wsum(Y, src, w, off, rows, out=None, accumulate=False):
    """out[j] (+)= sum_{e in [off[j], off[j+1])} w[e] * Y[src[e]]; out has Y's dtype"""
    dev = _dev(Y); _contig(Y); _contig(src); _contig(w); _contig(off)
    if out is None:
        out = torch.empty((rows, Y.shape[1]), dtype=Y.dtype, device=dev)
        accumulate = False
    check(_lib.lib().wavlm_rows_wsum(ptr(Y), dt(Y), ptr(src), ptr(w), ptr(off), ptr(out), dt(out), rows, Y.shape[1],
                                     int(bool(accumulate)), stream()), "wavlm_rows_wsum")
    return out


def bce_logits(logits, targets_u8, gscale, want_grad=True):
    """(out[2] = (mean BCE-with-logits, accuracy of logit >= 0), dlogits = gscale * (sigmoid - target) or None)"""
    dev = _dev(logits); _contig(logits); _contig(targets_u8)
    n = logits.numel()
    out = torch.empty(2, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if want_grad else None
    L = _lib.lib()
    need = L.wavlm_bce_workspace_bytes()
    ws = workspace(dev, need)
    check(L.wavlm_bce_logits(ptr(logits), ptr(targets_u8), ptr(dl), ptr(out), n, float(gscale), ptr(ws), need, stream()),
          "wavlm_bce_logits")
    return out, dl


# ------------------------------------------------------------------------------- Gumbel vector quantiser
def gumbel_vq_fwd(logits, G, V, tau, training, noise=None, seed=0):
    """logits [n, G*V] -> (idx int32 [n*G] (global code index g*V + k), ysoft fp32 [n*G, V] or None, out[2] =
    (prob_perplexity, code_perplexity), dA [G*V] = d prob_perplexity / d avg_probs)"""
    dev = _dev(logits); _contig(logits); _contig(noise)
    n = logits.shape[0]
    L = _lib.lib()
    rows = int(L.wavlm_gumbel_vq_partial_rows(n))
    ldp = (2 * G * V + 7) // 8 * 8   # wavlm_colsum sums 8-column granules: pad columns are zero and dropped below
    part = (torch.empty if ldp == 2 * G * V else torch.zeros)((rows, ldp), dtype=torch.float32, device=dev)
    idx = torch.empty(n * G, dtype=torch.int32, device=dev)
    ysoft = torch.empty((n * G, V), dtype=torch.float32, device=dev) if training else None
    check(L.wavlm_gumbel_vq_fwd(ptr(logits), dt(logits), ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, float(tau),
                                int(bool(training)), n, int(G), int(V), ptr(ysoft), ptr(idx), ptr(part), ldp, stream()),
          "wavlm_gumbel_vq_fwd")
    sums = colsum(part, torch.float32)[:2 * G * V]
    out = torch.empty(2, dtype=torch.float32, device=dev)
    dA = torch.empty(G * V, dtype=torch.float32, device=dev)
    check(L.wavlm_vq_perplexity(ptr(sums), n, int(G), int(V), ptr(out), ptr(dA), stream()), "wavlm_vq_perplexity")
    return idx, ysoft, out, dA


def gumbel_vq_bwd(logits, ysoft, dret, dA, dppl, G, V, tau):
    """dlogits [n, G*V] (dtype of logits); ysoft / dret None in eval mode, dppl None when the perplexity carries no gradient"""
    _dev(logits); _contig(dret)
    n = logits.shape[0]
    dl = torch.empty_like(logits)
    check(_lib.lib().wavlm_gumbel_vq_bwd(ptr(logits), dt(logits), ptr(ysoft), ptr(dret), ptr(dA), ptr(dppl), float(tau), n,
                                         int(G), int(V), ptr(dl), stream()), "wavlm_gumbel_vq_bwd")
    return dl


# ------------------------------------------------------------------------------------- utterance mixing
def mix_utterances(src, ops_flat, n_ops, op_begin, noise, normalize, out_dtype=torch.float32, eps=1e-5):
    """src fp32 [B, T] (left untouched) -> mixed batch [B, T] in out_dtype (fp32, or bf16 = the Trainer's waveform cast);
    ops_flat int32 [n_ops * 8], op_begin int32 [B + 1], noise fp32 or None (see include/wavlm_hip.h)"""
    dev = _dev(src); _contig(src)
    if src.dtype != torch.float32:
        raise TypeError("mix_utterances works on the fp32 collated waveform")
    B, T = src.shape
    dst = torch.empty_like(src)
    low = torch.empty((B, T), dtype=torch.bfloat16, device=dev) if out_dtype == torch.bfloat16 else None
    L = _lib.lib()
    need = L.wavlm_mix_workspace_bytes(B, T)
    ws = workspace(dev, need, "mix")
    check(L.wavlm_mix_utterances(ptr(src), ptr(dst), ptr(low), B, T, ptr(ops_flat) if n_ops else None, int(n_ops),
                                 ptr(op_begin), ptr(noise), int(bool(normalize)), float(eps), ptr(ws), need, stream()),
          "wavlm_mix_utterances")
    return low if low is not None else dst


# ------------------------------------------------------------------------------------ diarization head (csrc/diar.hip)
def diar_front(states, weights, T_out, subsampling=1, add=1e-6, eps=1e-5, out=None):
    """states: L + 1 tensors [B, T', D] (unit channel stride), weights fp32 [L + 1] (softmax applied) -> [B, T_out, D]:
    layer mix + add, InstanceNorm1d over time, every subsampling-th frame, linear interpolation to T_out frames"""
    s0 = states[0]
    dev = _dev(s0)
    if s0.dim() != 3 or any(s.shape != s0.shape or s.dtype != s0.dtype or s.device != dev or s.stride(2) != 1
                            or s.stride(1) < s.shape[2] for s in states):
        raise ValueError("states must share one shape [B, T', D], dtype and device and have unit channel stride")
    B, T, D = s0.shape
    n = len(states)
    if weights.numel() != n or weights.dtype != torch.float32 or weights.device != dev or not weights.is_contiguous():
        raise ValueError("weights must be %d contiguous fp32 values on the states' device" % n)
    if out is None:
        out = torch.empty((B, T_out, D), dtype=s0.dtype, device=dev)
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in states])
    sb = (C.c_int64 * n)(*[s.stride(0) for s in states])
    stt = (C.c_int64 * n)(*[s.stride(1) for s in states])
    check(_lib.lib().wavlm_diar_front(ptrs, sb, stt, n, dt(s0), ptr(weights), B, T, D, int(subsampling), int(T_out), ptr(out),
                                      dt(out), out.stride(0), out.stride(1), float(add), float(eps), stream()),
          "wavlm_diar_front")
    return out


def attn_plain_fwd(qkv, H, scale=None):
    """packed qkv [B, T, 3 * H * d] (d = 32) -> softmax(scale * Q K^T) V as [B, T, H * d]; scale defaults to 1 / sqrt(d)"""
    _dev(qkv)
    _contig(qkv)
    B, T, D3 = qkv.shape
    d = D3 // (3 * H)
    if d * 3 * H != D3:
        raise ValueError("qkv width %d is not 3 * %d heads * head_dim" % (D3, H))
    O = torch.empty((B, T, H * d), dtype=qkv.dtype, device=qkv.device)
    check(_lib.lib().wavlm_attn_plain_fwd(ptr(qkv), ptr(O), B, H, T, d, dt(qkv), float(scale if scale is not None else d ** -0.5),
                                          stream()), "wavlm_attn_plain_fwd[B=%d H=%d T=%d d=%d]" % (B, H, T, d))
    return O


def diar_estimate(z, S, E):
    """z [B, T, >= S + S * E] (logits | S vectors per frame) -> (activities fp32 [B, T, S], vectors [B, S, E])"""
    dev = _dev(z)
    B, T, ld = z.shape
    if z.stride(2) != 1 or z.stride(1) < ld:
        raise ValueError("expected unit channel stride")
    act = torch.empty((B, T, S), dtype=torch.float32, device=dev)
    vec = torch.empty((B, S, E), dtype=z.dtype, device=dev)
    check(_lib.lib().wavlm_diar_estimate(ptr(z), dt(z), z.stride(0), z.stride(1), B, T, int(S), int(E), ptr(act), ptr(vec), dt(vec),
                                         stream()), "wavlm_diar_estimate")
    return act, vec


# ------------------------------------------------------------------------------------ Transformer LM
def lm_logprob_supported(D, V, dtype):
    return bool(_lib.lib().wavlm_lm_logprob_supported(int(D), int(V), BF16 if dtype == torch.bfloat16 else F32))


def lm_logprob(x, w, target, want_lse=False):
    """x [R, D] (unit channel stride), w [V, D], target int32 [R] -> (logprob fp32 [R], lse fp32 [R] or None):
    logprob[r] = (w x_r)[target[r]] - logsumexp(w x_r), 0 for a negative target, NaN for one >= V.  The [R, V] logits never
    exist: the workspace is 12 bytes per (row, slab of 2048 entries)."""
    dev = _dev(x)
    R, D = x.shape
    V = w.shape[0]
    if x.dtype != w.dtype or w.shape[1] != D or x.stride(1) != 1 or w.stride(1) != 1:
        raise ValueError("x [R, D] and w [V, D] must share a dtype and D, with unit channel stride")
    if target.dtype != torch.int32 or target.numel() != R or not target.is_contiguous():
        raise ValueError("target must be a contiguous int32 tensor of %d entries" % R)
    logprob = torch.empty(R, dtype=torch.float32, device=dev)
    lse = torch.empty(R, dtype=torch.float32, device=dev) if want_lse else None
    if R == 0:
        return logprob, lse
    L = _lib.lib()
    need = L.wavlm_lm_logprob_workspace_bytes(R, V)
    ws = workspace(dev, need, "lm_logprob")
    check(L.wavlm_lm_logprob(ptr(x), x.stride(0), ptr(w), w.stride(0), dt(x), ptr(target), R, D, V, ptr(logprob), ptr(lse),
                             ptr(ws), need, stream()), "wavlm_lm_logprob[R=%d D=%d V=%d]" % (R, D, V))
    return logprob, lse


def attn_causal_fwd(qkv, H, lengths=None, scale=None):
    """packed qkv [B, T, 3 * H * d] (d = 32 or 64) -> causal softmax(scale * Q K^T) V as [B, T, H * d]; lengths int32 [B] on the
    device (rows at or beyond a length come back as zeros); scale defaults to 1 / sqrt(d)"""
    _dev(qkv)
    _contig(qkv)
    B, T, D3 = qkv.shape
    d = D3 // (3 * H)
    if d * 3 * H != D3:
        raise ValueError("qkv width %d is not 3 * %d heads * head_dim" % (D3, H))
    if lengths is not None and (lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_contiguous()
                                or lengths.device != qkv.device):
        raise ValueError("lengths must be a contiguous int32 tensor of %d entries on the device of qkv" % B)
    O = torch.empty((B, T, H * d), dtype=qkv.dtype, device=qkv.device)
    check(_lib.lib().wavlm_attn_causal_fwd(ptr(qkv), ptr(O), ptr(lengths), B, H, T, d, dt(qkv),
                                           float(scale if scale is not None else d ** -0.5), stream()),
          "wavlm_attn_causal_fwd[B=%d H=%d T=%d d=%d]" % (B, H, T, d))
    return O


def attn_step_supported(head_dim, dtype):
    return bool(_lib.lib().wavlm_attn_step_supported(int(head_dim), BF16 if dtype == torch.bfloat16 else F32))


def attn_step(qkv, kcache, vcache, slot, anc, lengths, H, max_length, scale=None):
    """one new token per row over a tree-shaped KV cache: qkv [R, 3 * H * d] packed q | k | v (d = 32 or 64), kcache / vcache
    [slots, H * d] (written at slot[r] by this call), slot int32 [R], anc int32 [R, >= max_length - 1] the slots of each row's
    ancestors in position order, lengths int32 [R] counting the row itself (<= 0: a row of zeros, nothing stored), max_length the
    largest of them -> softmax(scale * q [K[anc] ; k]^T) [V[anc] ; v] as [R, H * d]; scale defaults to 1 / sqrt(d).  No row may
    name a slot another row of the call writes."""
    dev = _dev(qkv)
    R, D3 = qkv.shape
    D = D3 // 3
    d = D // H
    if d * 3 * H != D3 or qkv.stride(1) != 1:
        raise ValueError("qkv width %d is not 3 * %d heads * head_dim with unit channel stride" % (D3, H))
    for name, c in (("kcache", kcache), ("vcache", vcache)):
        if c.dim() != 2 or c.shape[1] != D or c.stride(1) != 1 or c.dtype != qkv.dtype or c.device != qkv.device:
            raise ValueError("%s must be [slots, %d] of qkv's dtype on its device with unit channel stride" % (name, D))
    if kcache.shape[0] != vcache.shape[0] or kcache.stride(0) != vcache.stride(0):
        raise ValueError("kcache and vcache must have the same slots and row stride")
    for name, t in (("slot", slot), ("lengths", lengths)):
        if t.dtype != torch.int32 or t.numel() != R or not t.is_contiguous() or t.device != qkv.device:
            raise ValueError("%s must be a contiguous int32 tensor of %d entries on the device of qkv" % (name, R))
    if anc.dtype != torch.int32 or anc.dim() != 2 or anc.shape[0] != R or anc.shape[1] < max(1, int(max_length) - 1) or \
            (anc.shape[1] > 1 and anc.stride(1) != 1) or anc.device != qkv.device:
        raise ValueError("anc must be an int32 tensor [%d, >= max(1, max_length - 1)] on the device of qkv" % R)
    ld_anc = anc.stride(0) if R > 1 else anc.shape[1]
    O = torch.empty((R, D), dtype=qkv.dtype, device=dev)
    if R == 0:
        return O
    check(_lib.lib().wavlm_attn_step(ptr(qkv), qkv.stride(0), ptr(kcache), ptr(vcache), kcache.stride(0), kcache.shape[0],
                                     ptr(slot), ptr(anc), ld_anc, ptr(lengths), int(max_length), ptr(O), O.stride(0), R, H, d, dt(qkv),
                                     float(scale if scale is not None else d ** -0.5), stream()),
          "wavlm_attn_step[R=%d H=%d d=%d max_length=%d]" % (R, H, d, max_length))
    return O


# ------------------------------------------------------------------------------------ seq2seq decoding
def attn_cross_fwd_supported(head_dim, dtype):
    return bool(_lib.lib().wavlm_attn_cross_fwd_supported(int(head_dim), BF16 if dtype == torch.bfloat16 else F32))


def _i32(name, t, n, dev):
    if t is not None and (t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous() or t.device != dev):
        raise ValueError("%s must be a contiguous int32 tensor of %d entries on the device of the other arguments" % (name, n))


def attn_cross_fwd(q, kv, H, row_offsets, src_lengths=None, live=None, max_group=None, scale=None, out=None):
    """q [R, H * d] (d = 32 or 64, any row stride), kv [B, Ts, 2 * H * d] a frame's keys then its values (any batch and row
    stride), row_offsets int32 [B + 1]: rows row_offsets[b] .. row_offsets[b + 1] - 1 attend sentence b; src_lengths int32 [B]
    (None: Ts); live int32 [R] (None: all; <= 0: a row of zeros that reads nothing) -> softmax(scale * q K_b^T) V_b as [R, H * d].
    max_group: the largest group expected (sizes the grid; None: R); scale defaults to 1 / sqrt(d).  The rows of a sentence share
    one pass over its keys and values."""
    dev = _dev(q)
    if q.dim() != 2 or kv.dim() != 3 or q.stride(1) != 1 or kv.stride(2) != 1 or q.dtype != kv.dtype or kv.device != dev:
        raise ValueError("q [R, H * d] and kv [B, Ts, 2 * H * d] must share a dtype and a device, with unit channel stride")
    R, D = q.shape
    B, Ts, D2 = kv.shape
    d = D // H
    if d * H != D or D2 != 2 * D:
        raise ValueError("q width %d is not %d heads * head_dim, or kv width %d is not twice that" % (D, H, D2))
    _i32("row_offsets", row_offsets, B + 1, dev)
    _i32("src_lengths", src_lengths, B, dev)
    _i32("live", live, R, dev)
    if row_offsets is None:
        raise ValueError("row_offsets is needed")
    O = torch.empty((R, D), dtype=q.dtype, device=dev) if out is None else out
    if O.shape != (R, D) or O.dtype != q.dtype or O.stride(1) != 1 or O.device != dev:
        raise ValueError("out must be [%d, %d] of q's dtype on its device with unit channel stride" % (R, D))
    if R == 0:
        return O
    check(_lib.lib().wavlm_attn_cross_fwd(ptr(q), q.stride(0) if R > 1 else max(q.stride(0), D), ptr(kv),
                                          kv.stride(0) if B > 1 else max(kv.stride(0), Ts * kv.stride(1)), kv.stride(1),
                                          ptr(src_lengths), ptr(row_offsets), ptr(live), ptr(O),
                                          O.stride(0) if R > 1 else max(O.stride(0), D), R, B, Ts, H, d, dt(q),
                                          float(scale if scale is not None else d ** -0.5),
                                          int(max_group if max_group is not None else R), stream()),
          "wavlm_attn_cross_fwd[R=%d B=%d Ts=%d H=%d d=%d]" % (R, B, Ts, H, d))
    return O


def beam_step_supported(beam, V, B, dtype):
    return bool(_lib.lib().wavlm_beam_step_supported(int(beam), int(V), int(B), BF16 if dtype == torch.bfloat16 else F32))


class BeamState:
    """the device state wavlm_beam_step works on, for B sentences x `beam` rows and steps 0 .. max_len: cum, n_live, tokens,
    lengths, slots, two ancestor buffers, the tree (parent, token, score per slot), the finished lists and the counter of
    finished sentences.  Step 0's rows: row b * beam of every sentence is live, holds `bos`, slot b * beam, length 1."""

    def __init__(self, B, beam, max_len, bos, device):
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)  # noqa: E731
        self.B, self.beam, self.max_len = int(B), int(beam), int(max_len)
        R = self.B * self.beam
        self.tree_slots = (self.max_len + 2) * R
        self.cum = torch.zeros(R, dtype=torch.float32, device=device)
        self.n_live = torch.ones(self.B, dtype=torch.int32, device=device)
        first = torch.arange(R, device=device) % self.beam == 0
        self.tokens = torch.where(first, int(bos), 0).to(torch.int32)
        self.lengths = first.to(torch.int32)
        self.slots = torch.arange(R, dtype=torch.int32, device=device)
        self.ld_anc = self.max_len + 1
        self.anc = [i32(R, self.ld_anc), i32(R, self.ld_anc)]
        self.tree_parent = torch.full((self.tree_slots,), -1, dtype=torch.int32, device=device)
        self.tree_token = i32(self.tree_slots)
        self.tree_token[:R] = int(bos)
        self.tree_score = torch.zeros(self.tree_slots, dtype=torch.float32, device=device)
        self.fin_f = torch.zeros((self.B, self.beam, 3), dtype=torch.float32, device=device)
        self.fin_i = i32(self.B, self.beam, 2)
        self.n_fin = i32(self.B)
        self.finished = i32(1)
        self.ws = torch.zeros(int(_lib.lib().wavlm_beam_step_workspace_bytes(self.B, self.beam)), dtype=torch.uint8, device=device)
        self.step = 0

    def candidates(self):
        """the last step's candidates: (scores fp32 [B, 2 beam], flat indices int32 [B, 2 beam], counts int32 [B])"""
        n = self.B * 2 * self.beam
        return (self.ws[:4 * n].view(torch.float32).view(self.B, -1), self.ws[4 * n:8 * n].view(torch.int32).view(self.B, -1),
                self.ws[8 * n:8 * n + 4 * self.B].view(torch.int32))


def beam_step(logits, st, V, *, max_len, min_len, pad, unk, eos, unk_penalty=0.0, temperature=1.0, len_penalty=1.0,
              normalize_scores=True, step=None):
    """one search step over st (a BeamState): logits [B * beam, >= V] of this step's rows (fp32 or bf16, unit column stride);
    reads st.anc[step % 2], writes st.anc[(step + 1) % 2]; st.step goes up by one"""
    _dev(logits)
    step = st.step if step is None else int(step)
    if logits.dim() != 2 or logits.shape[0] != st.B * st.beam or logits.shape[1] < V or logits.stride(1) != 1:
        raise ValueError("logits must be [%d, >= %d] with unit column stride" % (st.B * st.beam, V))
    if step > st.max_len:
        raise ValueError("step %d is beyond the %d steps the state was made for" % (step, st.max_len))
    L = _lib.lib()
    check(L.wavlm_beam_step(ptr(logits), logits.stride(0), dt(logits), ptr(st.cum), ptr(st.n_live), ptr(st.tokens), ptr(st.lengths),
                            ptr(st.slots), ptr(st.anc[step % 2]), ptr(st.anc[(step + 1) % 2]), st.ld_anc, ptr(st.tree_parent),
                            ptr(st.tree_token), ptr(st.tree_score), st.tree_slots, ptr(st.fin_f), ptr(st.fin_i), ptr(st.n_fin),
                            ptr(st.finished), st.B, st.beam, int(V), step, int(max_len), int(min_len), int(pad), int(unk), int(eos),
                            float(unk_penalty), float(temperature), float(len_penalty), int(bool(normalize_scores)), ptr(st.ws),
                            st.ws.numel(), stream()),
          "wavlm_beam_step[B=%d beam=%d V=%d step=%d]" % (st.B, st.beam, V, step))
    st.step = step + 1


def beam_step_fused_supported(beam, V, B, dtype, lm_dtype=torch.float32):
    c = lambda d: BF16 if d == torch.bfloat16 else F32  # noqa: E731
    return bool(_lib.lib().wavlm_beam_step_fused_supported(int(beam), int(V), int(B), c(dtype), c(lm_dtype)))


def beam_step_fused(logits, st, V, *, max_len, min_len, pad, unk, eos, lm_logits=None, lm_weight=1.0, no_repeat_ngram_size=0,
                    unk_penalty=0.0, temperature=1.0, len_penalty=1.0, normalize_scores=True, step=None):
    """beam_step with shallow fusion and the n-gram blocker: lm_logits [B * beam, >= V] (fp32 or bf16, unit column stride; None:
    no LM) enters as lm_weight * log_softmax(lm_logits) before the NaN rule; no_repeat_ngram_size = n > 0 bans, per row, every
    token that would repeat an n-gram of the row's history (read from st's tree).  `logits` IS CONSUMED: with n > 0 the banned
    entries of the live rows are overwritten with -inf (nothing else is written; with n = 0 nothing is).  With lm_logits None
    and n = 0 the state after the call equals beam_step's bit for bit."""
    _dev(logits)
    step = st.step if step is None else int(step)
    R = st.B * st.beam
    if logits.dim() != 2 or logits.shape[0] != R or logits.shape[1] < V or logits.stride(1) != 1:
        raise ValueError("logits must be [%d, >= %d] with unit column stride" % (R, V))
    if lm_logits is not None and (lm_logits.dim() != 2 or lm_logits.shape[0] != R or lm_logits.shape[1] < V or
                                  lm_logits.stride(1) != 1 or lm_logits.device != logits.device):
        raise ValueError("lm_logits must be [%d, >= %d] with unit column stride on the device of logits" % (R, V))
    if step > st.max_len:
        raise ValueError("step %d is beyond the %d steps the state was made for" % (step, st.max_len))
    L = _lib.lib()
    check(L.wavlm_beam_step_fused(ptr(logits), logits.stride(0), dt(logits), ptr(lm_logits),
                                  lm_logits.stride(0) if lm_logits is not None else 0,
                                  dt(lm_logits) if lm_logits is not None else F32, float(lm_weight), int(no_repeat_ngram_size),
                                  ptr(st.cum), ptr(st.n_live), ptr(st.tokens), ptr(st.lengths), ptr(st.slots), ptr(st.anc[step % 2]),
                                  ptr(st.anc[(step + 1) % 2]), st.ld_anc, ptr(st.tree_parent), ptr(st.tree_token),
                                  ptr(st.tree_score), st.tree_slots, ptr(st.fin_f), ptr(st.fin_i), ptr(st.n_fin), ptr(st.finished),
                                  st.B, st.beam, int(V), step, int(max_len), int(min_len), int(pad), int(unk), int(eos),
                                  float(unk_penalty), float(temperature), float(len_penalty), int(bool(normalize_scores)),
                                  ptr(st.ws), st.ws.numel(), stream()),
          "wavlm_beam_step_fused[B=%d beam=%d V=%d step=%d n=%d]" % (st.B, st.beam, V, step, int(no_repeat_ngram_size)))
    st.step = step + 1


# ---------------------------------------------------------------------------------------------- CTC
def _ctc_view(logits):
    """(stride_b, stride_t) in elements of a [B, T, C]-indexed view with unit class stride"""
    if logits.dim() != 3:
        raise ValueError("logits: expected a [B, T, C] view, got %d dimensions" % logits.dim())
    if logits.shape[2] > 1 and logits.stride(2) != 1:
        raise ValueError("logits: the class axis must have unit stride")
    return logits.stride(0), logits.stride(1)


def ctc_supported(C, Lmax):
    return bool(_lib.lib().wavlm_ctc_supported(int(C), int(Lmax)))


def ctc_check_supported(C, Lmax):
    """NotImplementedError naming the argument that is beyond wavlm_ctc_supported; nothing is launched"""
    L = _lib.lib()
    if not L.wavlm_ctc_supported(int(C), 0):
        raise NotImplementedError("ctc_loss: C = %d classes is beyond the kernel's limit (wavlm_ctc_supported: C <= 1024)" % C)
    if not L.wavlm_ctc_supported(int(C), int(Lmax)):
        raise NotImplementedError("ctc_loss: L = %d labels in one target is beyond the kernel's limit (wavlm_ctc_supported: "
                                  "L <= 1023)" % Lmax)


def ctc_loss_fwd_bwd(logits, targets, target_offsets, n_targets, Lmax, input_lengths, blank, grad_out=None,
                     zero_infinity=False, dlogits=None):
    """wavlm_ctc_loss.  logits: a [B, T, C]-indexed view, fp32 or bf16, any batch / time strides (a T x B x C tensor is passed
    as its transpose(0, 1)) -- read in place.  targets int32 [n_targets] flat, target_offsets int32 [B + 1], input_lengths int32
    [B], all on the device; n_targets and Lmax are host integers.  grad_out fp32 [B] (None: ones).  Returns (nll fp32 [B],
    dlogits with the dtype, shape and strides of logits).  dlogits (optional): a view with exactly those strides to write into."""
    dev = _dev(logits)
    sb, st = _ctc_view(logits)
    B, T, Cn = logits.shape
    ctc_check_supported(Cn, Lmax)
    for name, t, n in (("targets", targets, n_targets), ("target_offsets", target_offsets, B + 1),
                       ("input_lengths", input_lengths, B)):
        if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous() or t.numel() < n:
            raise ValueError("%s: expected a contiguous int32 device tensor of at least %d elements" % (name, n))
    if grad_out is None:
        grad_out = torch.ones(B, dtype=torch.float32, device=dev)
    elif grad_out.dtype != torch.float32 or grad_out.numel() != B or not grad_out.is_contiguous():
        raise ValueError("grad_out: expected a contiguous fp32 tensor of B elements")
    if dlogits is None:
        dlogits = torch.empty_strided(logits.shape, logits.stride(), dtype=logits.dtype, device=dev)
    elif dlogits.shape != logits.shape or dlogits.stride() != logits.stride() or dlogits.dtype != logits.dtype:
        raise ValueError("dlogits: expected the shape, strides and dtype of logits")
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    L = _lib.lib()
    need = L.wavlm_ctc_workspace_bytes(B, T, int(Lmax))
    ws = workspace(dev, need, "ctc")
    check(L.wavlm_ctc_loss(ptr(logits), dt(logits), sb, st, B, T, Cn, ptr(targets), ptr(target_offsets), int(n_targets),
                           int(Lmax), ptr(input_lengths), int(blank), int(bool(zero_infinity)), ptr(grad_out), ptr(nll),
                           ptr(dlogits), ptr(ws), need, stream()), "wavlm_ctc_loss")
    return nll, dlogits


def ctc_greedy(logits, input_lengths, blank):
    """wavlm_ctc_greedy on a [B, T, C]-indexed view: (tokens int32 [B, T], counts int32 [B]) on the device"""
    dev = _dev(logits)
    sb, st = _ctc_view(logits)
    B, T, Cn = logits.shape
    if input_lengths.dtype != torch.int32 or input_lengths.device != dev or input_lengths.numel() != B:
        raise ValueError("input_lengths: expected an int32 device tensor of B elements")
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    check(_lib.lib().wavlm_ctc_greedy(ptr(logits), dt(logits), sb, st, B, T, Cn, ptr(input_lengths.contiguous()), int(blank),
                                      ptr(tokens), ptr(counts), stream()), "wavlm_ctc_greedy")
    return tokens, counts


def ctc_score_supported(T, Lt):
    return bool(_lib.lib().wavlm_ctc_score_supported(int(T), int(Lt)))


def ctc_score(logits, input_lengths, targets, pad, eos, blank, cls, each_token_a_word=False):
    """wavlm_ctc_score on a [B, T, C]-indexed view (the rules of ctc_greedy): the greedy decode and the error counts of every sample
    in one launch.  targets int32 [B, Lt] padded, cls uint8 [C] (0 DROP, 1 SEP, 2 LETTER), both on the device.  Returns
    (counts int32 [B, 4] = c_err, c_len, w_err, w_len; tokens int32 [B, T]; token_counts int32 [B]), all on the device."""
    dev = _dev(logits)
    sb, st = _ctc_view(logits)
    B, T, Cn = logits.shape
    if input_lengths.dtype != torch.int32 or input_lengths.device != dev or input_lengths.numel() != B:
        raise ValueError("input_lengths: expected an int32 device tensor of B elements")
    if targets.dim() != 2 or targets.shape[0] != B or targets.dtype != torch.int32 or targets.device != dev \
            or not targets.is_contiguous():
        raise ValueError("targets: expected a contiguous int32 device tensor [B, Lt]")
    if cls.dtype != torch.uint8 or cls.device != dev or cls.numel() != Cn or not cls.is_contiguous():
        raise ValueError("cls: expected a contiguous uint8 device tensor of C = %d elements" % Cn)
    Lt = targets.shape[1]
    L = _lib.lib()
    if not L.wavlm_ctc_score_supported(T, Lt):
        raise NotImplementedError("ctc_score: T = %d frames, Lt = %d target columns is beyond the kernel's limit "
                                  "(wavlm_ctc_score_supported: T >= 1, Lt <= 1024)" % (T, Lt))
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    token_counts = torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    need = L.wavlm_ctc_score_workspace_bytes(B, T, Lt)
    # not ops.workspace(): a few hundred KiB a call, and a grow-only buffer kept for the life of the process would be held for
    # a call made once per validation batch (the caching allocator hands the same block out again; launches are stream-ordered)
    ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    check(L.wavlm_ctc_score(ptr(logits), dt(logits), sb, st, B, T, Cn, ptr(input_lengths.contiguous()), int(blank),
                            ptr(targets) if Lt else None, Lt, int(pad), int(eos), ptr(cls), int(bool(each_token_a_word)),
                            ptr(tokens), ptr(token_counts), ptr(counts), ptr(ws), need, stream()), "wavlm_ctc_score")
    return counts, tokens, token_counts


def ctc_align_check_supported(Lmax):
    """NotImplementedError naming the value that is beyond wavlm_ctc_align_supported; nothing is launched"""
    if not _lib.lib().wavlm_ctc_align_supported(int(Lmax)):
        raise NotImplementedError("ctc_align: L = %d labels in one target is beyond the kernel's limit "
                                  "(wavlm_ctc_align_supported: L <= 1023)" % Lmax)


def ctc_align(logits, targets, target_offsets, n_targets, Lmax, input_lengths, blank, ws=None):
    """wavlm_ctc_align on a [B, T, C]-indexed view (the rules of ctc_loss_fwd_bwd for logits, targets, target_offsets and
    input_lengths).  Returns (frames int32 [B, T], spans int32 [B, Lmax, 2], token_scores fp32 [B, Lmax], score fp32 [B]) on the
    device.  ws (optional): a uint8 device tensor to use as the workspace -- it starts with the kernel's uint64 [B, 4] clock
    stamps, which tools/ctc_align_bench.py reads."""
    dev = _dev(logits)
    sb, st = _ctc_view(logits)
    B, T, Cn = logits.shape
    Lmax = int(Lmax)
    ctc_align_check_supported(Lmax)
    for name, t, n in (("targets", targets, n_targets), ("target_offsets", target_offsets, B + 1),
                       ("input_lengths", input_lengths, B)):
        if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous() or t.numel() < n:
            raise ValueError("%s: expected a contiguous int32 device tensor of at least %d elements" % (name, n))
    frames = torch.empty((B, T), dtype=torch.int32, device=dev)
    spans = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    token_scores = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    L = _lib.lib()
    need = L.wavlm_ctc_align_workspace_bytes(B, T, Lmax)
    if ws is None:
        # not ops.workspace(), for the reason given at ctc_score
        ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    elif ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous():
        raise ValueError("ws: expected a contiguous uint8 device tensor")
    check(L.wavlm_ctc_align(ptr(logits), dt(logits), sb, st, B, T, Cn, ptr(targets) if n_targets else None, ptr(target_offsets),
                            int(n_targets), Lmax, ptr(input_lengths), int(blank), ptr(frames), ptr(spans) if Lmax else None,
                            ptr(token_scores) if Lmax else None, ptr(score), ptr(ws), ws.numel(), stream()), "wavlm_ctc_align")
    return frames, spans, token_scores, score


def ctc_beam_check_supported(C, beam, beam_tokens, lm_order):
    """NotImplementedError naming the argument that is beyond wavlm_ctc_beam_supported; nothing is launched"""
    L = _lib.lib()
    C, beam, beam_tokens, lm_order = int(C), int(beam), int(beam_tokens), int(lm_order)
    if not L.wavlm_ctc_beam_supported(C, 1, 1, 0):
        raise NotImplementedError("ctc_beam: C = %d classes is beyond the kernel's limit (wavlm_ctc_beam_supported: C <= 1024)" % C)
    if not L.wavlm_ctc_beam_supported(C, beam, 1, 0):
        raise NotImplementedError("ctc_beam: beam = %d is beyond the kernel's limit (wavlm_ctc_beam_supported: 1 <= beam <= 512)"
                                  % beam)
    if not L.wavlm_ctc_beam_supported(C, 1, 1, lm_order):
        raise NotImplementedError("ctc_beam: lm order = %d is beyond the kernel's limit (wavlm_ctc_beam_supported: order <= 6)"
                                  % lm_order)
    if not L.wavlm_ctc_beam_supported(C, beam, beam_tokens, lm_order):
        raise NotImplementedError("ctc_beam: beam_size_token = %d with beam = %d is beyond the kernel's limit "
                                  "(wavlm_ctc_beam_supported: beam x min(beam_size_token, C) <= 16384)" % (beam_tokens, beam))


def ctc_beam(logits, input_lengths, blank, sil, lm, beam, beam_tokens, beam_threshold, lm_weight, sil_weight, nbest,
             normalized=False):
    """wavlm_ctc_beam on a [B, T, C]-indexed view (the rules of ctc_greedy): the lexicon-free beam search of every sample in one
    launch.  lm: a ctc_lm.NgramLM (its tables are put on the device once) or None.  Returns (tokens int32 [B, nbest, T], counts
    int32 [B, nbest], scores fp32 [B, nbest], n_hyp int32 [B]), all on the device."""
    dev = _dev(logits)
    sb, st = _ctc_view(logits)
    B, T, Cn = logits.shape
    if input_lengths.dtype != torch.int32 or input_lengths.device != dev or input_lengths.numel() != B:
        raise ValueError("input_lengths: expected an int32 device tensor of B elements")
    beam, beam_tokens, nbest = int(beam), int(beam_tokens), int(nbest)
    if beam_tokens < 1:
        raise ValueError("beam_tokens must be at least 1")
    beam_tokens = min(beam_tokens, Cn)
    ctc_beam_check_supported(Cn, beam, beam_tokens, lm.order if lm is not None else 0)
    if not 1 <= nbest <= beam:
        raise ValueError("nbest: expected 1 .. beam = %d" % beam)
    if T < 1:
        raise ValueError("logits: expected at least one frame")
    if lm is not None:
        if len(lm.tok_word) < Cn:
            raise ValueError("lm: its symbol map has %d entries, the logits have C = %d classes" % (len(lm.tok_word), Cn))
        t = lm.to(dev)
        tabs = [ptr(t[k]) for k in ("child_off", "child_word", "child_logp", "child_next", "node_backoff", "node_suffix",
                                    "tok_word")]
        sizes = [len(lm), len(lm.child_word), int(lm.start), int(lm.eos_word), int(lm.order)]
    else:
        tabs, sizes = [None] * 7, [0, 0, 0, 0, 0]
    tokens = torch.empty((B, nbest, T), dtype=torch.int32, device=dev)
    counts = torch.empty((B, nbest), dtype=torch.int32, device=dev)
    scores = torch.empty((B, nbest), dtype=torch.float32, device=dev)
    n_hyp = torch.empty(B, dtype=torch.int32, device=dev)
    L = _lib.lib()
    need = L.wavlm_ctc_beam_workspace_bytes(B, T, beam)
    # not ops.workspace(), for the reason given at ctc_score: up to tens of MiB for a call made once per decoded batch
    ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    check(L.wavlm_ctc_beam(ptr(logits), dt(logits), sb, st, B, T, Cn, ptr(input_lengths.contiguous()), int(blank), int(sil),
                           int(bool(normalized)), *tabs, *sizes, beam, beam_tokens, float(beam_threshold), float(lm_weight),
                           float(sil_weight), nbest, ptr(tokens), ptr(counts), ptr(scores), ptr(n_hyp), ptr(ws), need, stream()),
          "wavlm_ctc_beam")
    return tokens, counts, scores, n_hyp


def ctc_lexbeam_max_beam(C, width, lm_order, lex_nodes):
    """the largest beam wavlm_ctc_lexbeam_supported admits for these sizes (0: none), found by probing it"""
    ok = _lib.lib().wavlm_ctc_lexbeam_supported
    lo, hi = 0, 1 << 20                    # supported(lo) (or lo = 0), not supported(hi); support is monotone in the beam
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(int(C), mid, int(width), int(lm_order), int(lex_nodes)):
            lo = mid
        else:
            hi = mid
    return lo


def ctc_lexbeam_check_supported(C, beam, width, lm_order, lex_nodes):
    """NotImplementedError naming the argument that is beyond wavlm_ctc_lexbeam_supported; nothing is launched"""
    L = _lib.lib()
    C, beam, width, lm_order, lex_nodes = int(C), int(beam), int(width), int(lm_order), int(lex_nodes)
    ok = L.wavlm_ctc_lexbeam_supported
    if not ok(C, 1, 1, 0, 1):
        raise NotImplementedError("ctc_lexbeam: C = %d classes is beyond the kernel's limit (wavlm_ctc_lexbeam_supported: C <= 1024)"
                                  % C)
    if not ok(C, beam, 1, 0, 1):
        raise NotImplementedError("ctc_lexbeam: beam = %d is beyond the kernel's limit (wavlm_ctc_lexbeam_supported: 1 <= beam <= "
                                  "512)" % beam)
    if not ok(C, 1, 1, lm_order, 1):
        raise NotImplementedError("ctc_lexbeam: lm order = %d is beyond the kernel's limit (wavlm_ctc_lexbeam_supported: order <= "
                                  "6)" % lm_order)
    if not ok(C, 1, 1, 0, lex_nodes):
        raise NotImplementedError("ctc_lexbeam: lexicon of %d trie nodes is beyond the kernel's limit "
                                  "(wavlm_ctc_lexbeam_supported: nodes <= 2^21)" % lex_nodes)
    if not ok(C, beam, width, lm_order, lex_nodes):
        raise NotImplementedError("ctc_lexbeam: beam = %d with this lexicon and beam_size_token (at most %d candidates per "
                                  "hypothesis and frame) is beyond the kernel's limit (wavlm_ctc_lexbeam_supported admits beam <= "
                                  "%d here)" % (beam, width, ctc_lexbeam_max_beam(C, width, lm_order, lex_nodes)))


def ctc_lexbeam(logits, input_lengths, blank, sil, lexicon, beam, beam_tokens, beam_threshold, lm_weight, word_score, unk_score,
                sil_weight, nbest, normalized=False):
    """wavlm_ctc_lexbeam on a [B, T, C]-indexed view (the rules of ctc_greedy): the lexicon-constrained beam search of every
    sample in one launch.  lexicon: a ctc_lexicon.Lexicon (its tables and those of its .lm are put on the device once).  Returns
    (tokens int32 [B, nbest, T], counts int32 [B, nbest], scores fp32 [B, nbest], n_hyp int32 [B], words int32 [B, nbest, T],
    word_counts int32 [B, nbest]), all on the device."""
    dev = _dev(logits)
    sb, st = _ctc_view(logits)
    B, T, Cn = logits.shape
    if input_lengths.dtype != torch.int32 or input_lengths.device != dev or input_lengths.numel() != B:
        raise ValueError("input_lengths: expected an int32 device tensor of B elements")
    beam, beam_tokens, nbest = int(beam), int(beam_tokens), int(nbest)
    if beam_tokens < 1:
        raise ValueError("beam_tokens must be at least 1")
    beam_tokens = min(beam_tokens, Cn)
    lm = lexicon.lm
    width = lexicon.width(beam_tokens, float(unk_score) > -math.inf)
    ctc_lexbeam_check_supported(Cn, beam, width, lm.order if lm is not None else 0, len(lexicon))
    if not 1 <= nbest <= beam:
        raise ValueError("nbest: expected 1 .. beam = %d" % beam)
    if T < 1:
        raise ValueError("logits: expected at least one frame")
    if len(lexicon.child_tok) and int(lexicon.child_tok.max()) >= Cn:
        raise ValueError("lexicon: it spells with token %d, the logits have C = %d classes" % (int(lexicon.child_tok.max()), Cn))
    if lm is not None:
        t = lm.to(dev)
        tabs = [ptr(t[k]) for k in ("child_off", "child_word", "child_logp", "child_next", "node_backoff", "node_suffix",
                                    "tok_word")]
        sizes = [len(lm), len(lm.child_word), int(lm.start), int(lm.eos_word), int(lm.order)]
    else:
        tabs, sizes = [None] * 7, [0, 0, 0, 0, 0]
    x = lexicon.to(dev)
    ltabs = [ptr(x[k]) for k in ("child_off", "child_tok", "child_node", "node_max", "label_off", "label_word")]
    lsizes = [len(lexicon), len(lexicon.child_tok), len(lexicon.label_word), len(lexicon.words), width, int(lexicon.unk_word)]
    tokens = torch.empty((B, nbest, T), dtype=torch.int32, device=dev)
    words = torch.empty((B, nbest, T), dtype=torch.int32, device=dev)
    counts = torch.empty((B, nbest), dtype=torch.int32, device=dev)
    word_counts = torch.empty((B, nbest), dtype=torch.int32, device=dev)
    scores = torch.empty((B, nbest), dtype=torch.float32, device=dev)
    n_hyp = torch.empty(B, dtype=torch.int32, device=dev)
    L = _lib.lib()
    need = L.wavlm_ctc_lexbeam_workspace_bytes(B, T, beam, width)
    # not ops.workspace(), for the reason given at ctc_score
    ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    check(L.wavlm_ctc_lexbeam(ptr(logits), dt(logits), sb, st, B, T, Cn, ptr(input_lengths.contiguous()), int(blank), int(sil),
                              int(bool(normalized)), *tabs, *sizes, *ltabs, *lsizes, beam, beam_tokens, float(beam_threshold),
                              float(lm_weight), float(word_score), float(unk_score), float(sil_weight), nbest, ptr(tokens),
                              ptr(counts), ptr(scores), ptr(n_hyp), ptr(words), ptr(word_counts), ptr(ws), need, stream()),
          "wavlm_ctc_lexbeam")
    return tokens, counts, scores, n_hyp, words, word_counts
