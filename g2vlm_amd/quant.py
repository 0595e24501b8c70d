"""Weight-only FP8 for the decode step: OCP e4m3fn codes with one power-of-two scale per output row.

    scale[n] = 2^ceil(log2(amax[n] / 448))      (a zero row: 1)
    q[n][k]  = RNE_e4m3fn(w[n][k] / scale[n])   (|w / scale| <= 448, so no NaN code 0x7F / 0xFF is ever produced)

`w` is the bf16-rounded weight the engine holds.  Because the scale is a power of two, q * scale is exactly a bf16 value
(three mantissa bits, an exponent bf16 has): an engine that streams (q, scale) is, to the bit, a bf16 engine on
dequantize_rows(q, scale), and dequantize(quantize(dq)) == dq.  The quantiser works row by row, so it commutes with every row
permutation (weights.interleave_gate_up) and with the row-wise concatenation of q / k / v.  Host code; runs once when
Engine.decode_weights is first set to "fp8".
"""
import torch

E4M3_MAX = 448.0


def quantize_rows_e4m3(w):
    """w [N, K] (bf16, or anything that rounds to it) -> (q uint8 [N, K] e4m3fn codes, scale fp32 [N] powers of two)."""
    assert w.dim() == 2
    w32 = w.detach().to("cpu").to(torch.bfloat16).to(torch.float32)
    amax = w32.abs().amax(dim=1).to(torch.float64)
    mant, exp = torch.frexp(amax / E4M3_MAX)                 # amax / 448 = mant * 2^exp, mant in [0.5, 1)
    exp = torch.where(mant == 0.5, exp - 1, exp)             # ceil(log2(.)): an exact power of two keeps its own exponent
    scale = torch.ldexp(torch.ones_like(amax), exp.clamp(-126, 127))     # a normal fp32 number
    scale = torch.where(amax > 0, scale, torch.ones_like(scale)).to(torch.float32)
    q = (w32 / scale[:, None]).to(torch.float8_e4m3fn)       # power-of-two division: exact; the cast rounds to nearest even
    return q.view(torch.uint8).contiguous(), scale.contiguous()


def dequantize_rows(q, scale):
    """(q uint8 [N, K], scale fp32 [N]) -> bf16 [N, K], exactly q * scale."""
    return (q.view(torch.float8_e4m3fn).to(torch.float32) * scale.to(torch.float32)[:, None]).to(torch.bfloat16)
