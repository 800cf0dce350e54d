"""Float64 emulations of the screen values (shared by test_gpu_kernels.py and test_gpu_screen_hits.py).

bf16 screen: the product of the bf16-rounded, fp64-normalised operands.
int8 screen: S_q S_g (q8 . c8) + e_g kq from the device's own steps and residual norms (Mi355Index.debug_i8_state), with
the rows and queries quantised here in float64.
"""

import numpy as np


def bf16_round(x: np.ndarray) -> np.ndarray:
    """numpy emulation of round-to-nearest-even fp32 -> bf16 -> fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def unit_rows64(x: np.ndarray) -> np.ndarray:
    """the rows of x, normalised in float64 (a zero row becomes NaN)"""
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.linalg.norm(x, axis=1, keepdims=True)


def cos64(Q: np.ndarray, sub: np.ndarray) -> np.ndarray:
    """exact cosines [B, rows] in float64"""
    return unit_rows64(Q) @ unit_rows64(sub).T


def e64_bf16(Q: np.ndarray, sub: np.ndarray) -> np.ndarray:
    """bf16 screen values [B, rows]: bf16(q_hat) . bf16(c_hat), accumulated in float64"""
    with np.errstate(invalid="ignore"):
        ch = bf16_round(unit_rows64(sub).astype(np.float32)).astype(np.float64)
        qh = bf16_round(unit_rows64(Q).astype(np.float32)).astype(np.float64)
    return qh @ ch.T


def e64_i8(Q: np.ndarray, sub: np.ndarray, sq, kq, step_rows, err_rows):
    """int8 screen values [B, rows] and the size of one accumulator unit [B, rows].  sq, kq: [B] from debug_i8_state;
    step_rows, err_rows: the group constants S_g, e_g of every row of `sub` (its group's, repeated)."""
    sq, kq, sg, eg = (np.asarray(x, dtype=np.float64) for x in (sq, kq, step_rows, err_rows))
    qh = unit_rows64(Q)
    ch = unit_rows64(sub)
    with np.errstate(invalid="ignore", divide="ignore"):
        q8 = np.clip(np.rint(qh / sq[:, None]), -127, 127)
        c8 = np.clip(np.rint(ch / sg[:, None]), -127, 127)
    unit = sq[:, None] * sg[None, :]
    return (q8 @ c8.T) * unit + kq[:, None] * eg[None, :], unit
