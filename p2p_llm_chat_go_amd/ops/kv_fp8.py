"""FP8 KV cache ops: quantising RoPE + KV write and paged attention over e4m3 pages.

Cache format (per layer, for K and for V; ``engine/kv_cache.py`` with ``kv_dtype="fp8"``):

    codes  ``[num_pages, n_kv_heads, PAGE=64, 128]`` ``torch.float8_e4m3fn`` (OCP e4m3)
    scales ``[num_pages, n_kv_heads, PAGE=64]`` fp32, one per (token, kv head) row

For a row x (K after RoPE, V as projected): ``s = amax(|x|) / 448`` (1 for a zero row),
``code = e4m3_rne(x / s)``, ``dequant = float(code) * s``.  GPU tensors run
``csrc/kernels/kv_fp8_write.hip`` / ``kv_fp8_attention.hip`` / ``kv_fp8_flash_prefill.hip``
(prompt chunks, ``flash_prefill_fp8``); CPU tensors the PyTorch reference of the same rule.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .attention import HEAD_DIM, PAGE, attn_workspace
from .gemm import FP8_MAX, rope_row_perm

F8 = torch.float8_e4m3fn


def quantize_kv_rows(x: torch.Tensor):
    """Reference quantiser: rows ``[..., 128]`` -> (codes e4m3 ``[..., 128]``, scales fp32
    ``[...]``)."""
    x = x.float()
    s = x.abs().amax(-1) / FP8_MAX
    s = torch.where(s > 0, s, torch.ones_like(s))
    codes = (x / s[..., None]).clamp(-FP8_MAX, FP8_MAX).to(F8)
    return codes, s


def dequantize_kv(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return codes.float() * scale.float()[..., None]


def _u8(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8)  # indexing ops are not defined on the 8-bit float dtype


def rope_cache_fp8_ref(qkv, pos, slots, cos_sin, n_heads, n_kv, q_out, k_codes, v_codes, k_scale,
                       v_scale):
    T, D = qkv.shape[0], HEAD_DIM
    nat = torch.empty_like(qkv)
    nat[:, rope_row_perm(n_heads + 2 * n_kv).to(qkv.device)] = qkv  # back to natural dim order
    x = nat.view(T, n_heads + 2 * n_kv, D).float()
    cs = cos_sin[pos.long()]  # [T, 64, 2]
    c, s = cs[..., 0][:, None, :], cs[..., 1][:, None, :]
    qk = x[:, :n_heads + n_kv]
    x1, x2 = qk[..., :D // 2], qk[..., D // 2:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    q_out.view(T, n_heads, D).copy_(rot[:, :n_heads].to(q_out.dtype))
    keep = slots >= 0
    sl = slots[keep].long()
    page, off = sl // PAGE, sl % PAGE
    for rows, codes, scale in ((rot[keep, n_heads:], k_codes, k_scale),
                               (x[keep, n_heads + n_kv:], v_codes, v_scale)):
        cq, sq = quantize_kv_rows(rows)  # [Tk, n_kv, 128], [Tk, n_kv]
        _u8(codes)[page, :, off] = _u8(cq)
        scale[page, :, off] = sq
    return q_out


def rope_cache_fp8(qkv: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor,
                   cos_sin: torch.Tensor, n_heads: int, n_kv: int, q_out: torch.Tensor,
                   k_codes: torch.Tensor, v_codes: torch.Tensor, k_scale: torch.Tensor,
                   v_scale: torch.Tensor) -> torch.Tensor:
    """qkv: ``[T, (n_heads + 2 n_kv) * 128]`` bf16 in ``rope_row_perm`` column order (the
    EPI_STORE output of the engine's permuted qkv projection).  Rotated q -> ``q_out`` in
    natural head-dim order; K (rotated) and V are quantised into the code pages and scale
    planes at ``slots[t]`` (< 0: the row writes only q)."""
    T = qkv.shape[0]
    assert k_codes.dtype == F8 and v_codes.dtype == F8 and k_scale.dtype == torch.float32
    if qkv.device.type != "cuda":
        return rope_cache_fp8_ref(qkv, pos, slots, cos_sin, n_heads, n_kv, q_out, k_codes,
                                  v_codes, k_scale, v_scale)
    assert qkv.stride(1) == 1 and q_out.stride(1) == 1
    _lib.check(_lib.lib().p2p_rope_cache_fp8(
        qkv.data_ptr(), qkv.stride(0), pos.data_ptr(), slots.data_ptr(), cos_sin.data_ptr(), T,
        n_heads, n_kv, HEAD_DIM, q_out.data_ptr(), q_out.stride(0), k_codes.data_ptr(),
        v_codes.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(),
        _lib.stream_ptr(qkv.device)), "rope_cache_fp8")
    return q_out


def _gather_fp8(codes, scale, bt_row, ctx):
    """Dequantised rows of keys 0 .. ctx-1, every kv head: [ctx, n_kv, 128] fp32."""
    pos = torch.arange(ctx, device=codes.device)
    pages = bt_row[pos // PAGE].long()
    return dequantize_kv(_u8(codes)[pages, :, pos % PAGE].view(F8), scale[pages, :, pos % PAGE])


def paged_attention_fp8_ref(q, k_codes, v_codes, k_scale, v_scale, block_tables, row_bt, ctx_lens,
                            n_heads, n_kv, scale, out):
    """fp32 softmax attention over the dequantised cache."""
    R = q.shape[0]
    G = n_heads // n_kv
    qv = q.view(R, n_kv, G, HEAD_DIM).float()
    res = torch.empty(R, n_kv, G, HEAD_DIM, dtype=torch.float32, device=q.device)
    for r in range(R):
        ctx = int(ctx_lens[r])
        bt_row = block_tables[int(row_bt[r]) if row_bt is not None else r]
        K = _gather_fp8(k_codes, k_scale, bt_row, ctx)
        V = _gather_fp8(v_codes, v_scale, bt_row, ctx)
        p = torch.softmax(torch.einsum("hgd,chd->hgc", qv[r], K) * scale, dim=-1)
        res[r] = torch.einsum("hgc,chd->hgd", p, V)
    out.view(R, n_kv, G, HEAD_DIM).copy_(res.to(out.dtype))
    return out


def paged_attention_fp8(q: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor,
                        k_scale: torch.Tensor, v_scale: torch.Tensor, block_tables: torch.Tensor,
                        row_bt: torch.Tensor | None, ctx_lens: torch.Tensor, n_heads: int,
                        n_kv: int, max_ctx: int, out: torch.Tensor | None = None,
                        workspace: tuple | None = None, scale: float | None = None) -> torch.Tensor:
    """``ops.paged_attention`` over FP8 pages: q ``[R, n_heads*128]`` bf16 -> out of the same
    shape; row r attends ``ctx_lens[r]`` keys of block-table row ``row_bt[r]`` (None: row r)."""
    R = q.shape[0]
    if scale is None:
        scale = 1.0 / math.sqrt(HEAD_DIM)
    if out is None:
        out = torch.empty(R, n_heads * HEAD_DIM, device=q.device, dtype=q.dtype)
    assert k_codes.dtype == F8 and v_codes.dtype == F8 and k_scale.dtype == torch.float32
    if q.device.type != "cuda":
        return paged_attention_fp8_ref(q, k_codes, v_codes, k_scale, v_scale, block_tables, row_bt,
                                       ctx_lens, n_heads, n_kv, scale, out)
    if workspace is None:
        workspace = attn_workspace(R, n_heads, max_ctx, q.device)
    po, pml = workspace
    n_chunks = -(-int(max_ctx) // 256)
    if n_chunks > 1 and (po is None or po.numel() < R * n_heads * n_chunks * HEAD_DIM
                         or pml.numel() < R * n_heads * n_chunks * 2):
        raise ValueError("paged_attention_fp8: workspace too small for max_ctx=%d" % max_ctx)
    _lib.check(_lib.lib().p2p_paged_attention_fp8(
        q.data_ptr(), q.stride(0), k_codes.data_ptr(), v_codes.data_ptr(), k_scale.data_ptr(),
        v_scale.data_ptr(), block_tables.data_ptr(), block_tables.stride(0), _lib.ptr(row_bt),
        ctx_lens.data_ptr(), R, n_heads, n_kv, HEAD_DIM, float(scale), int(max_ctx),
        out.data_ptr(), out.stride(0), _lib.ptr(po), _lib.ptr(pml), _lib.stream_ptr(q.device)),
        "paged_attention_fp8")
    return out


def flash_prefill_fp8(q: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor,
                      k_scale: torch.Tensor, v_scale: torch.Tensor, block_tables: torch.Tensor,
                      tiles: torch.Tensor, n_heads: int, n_kv: int,
                      out: torch.Tensor | None = None, scale: float | None = None,
                      tiles_host: torch.Tensor | None = None, *, qtile: int) -> torch.Tensor:
    """``ops.flash_prefill`` over FP8 pages (``csrc/kernels/kv_fp8_flash_prefill.hip``): causal
    MFMA attention for query tiles cut by ``prefill_tiles(seq, pos, qtile)`` with
    ``qtile = flash_tile(n_heads, n_kv, rows, kv_dtype="fp8")`` = 256 / (n_heads / n_kv); there
    is no 16-token FP8 kernel.  Same result as :func:`paged_attention_fp8` with one row per
    prompt token (ctx = pos + 1), reading each page once per tile instead of once per row."""
    if qtile is None or qtile < 1:
        raise ValueError("flash_prefill_fp8: qtile (the prefill_tiles width) is required")
    if tiles_host is not None and tiles_host.numel() and int(tiles_host[:, 1].max()) > qtile:
        raise ValueError("flash_prefill_fp8: tiles are wider than qtile=%d" % qtile)
    R = q.shape[0]
    if scale is None:
        scale = 1.0 / math.sqrt(HEAD_DIM)
    if out is None:
        out = torch.empty(R, n_heads * HEAD_DIM, device=q.device, dtype=q.dtype)
    assert k_codes.dtype == F8 and v_codes.dtype == F8 and k_scale.dtype == torch.float32
    if q.device.type != "cuda":
        th = (tiles_host if tiles_host is not None else tiles).cpu()
        row_bt = torch.empty(R, dtype=torch.int32)
        ctx = torch.empty(R, dtype=torch.int32)
        for r0, n, s, p0 in th.tolist():
            row_bt[r0:r0 + n] = s
            ctx[r0:r0 + n] = torch.arange(p0 + 1, p0 + n + 1, dtype=torch.int32)
        return paged_attention_fp8_ref(q, k_codes, v_codes, k_scale, v_scale, block_tables,
                                       row_bt, ctx, n_heads, n_kv, scale, out)
    G = n_heads // n_kv
    if n_heads % n_kv or G not in (1, 2, 4, 8) or qtile * G != 256:
        raise ValueError("flash_prefill_fp8: needs n_heads / n_kv in (1, 2, 4, 8) and tiles of "
                         "256 / (n_heads / n_kv) tokens, got %d / %d heads, qtile=%d"
                         % (n_heads, n_kv, qtile))
    assert q.stride(1) == 1 and out.stride(1) == 1
    _lib.check(_lib.lib().p2p_flash_prefill_fp8(
        q.data_ptr(), q.stride(0), k_codes.data_ptr(), v_codes.data_ptr(), k_scale.data_ptr(),
        v_scale.data_ptr(), block_tables.data_ptr(), block_tables.stride(0), tiles.data_ptr(),
        tiles.shape[0], n_heads, n_kv, HEAD_DIM, float(scale), out.data_ptr(), out.stride(0),
        _lib.stream_ptr(q.device)), "flash_prefill_fp8")
    return out
