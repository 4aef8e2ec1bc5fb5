"""float64 models of the pixel reconstruction filters (include/rtx.h), shared by the GPU tests: the filtered fold of
rtx_render_passes_filtered over given pass frames and weight tables, and a frame reconstructed with a filter from
a supersampled one."""
import math

import numpy as np

TAPS = 5


def f_eval(kind, d, r, a=2.0):
    """f(d) of the header on a float64 array d (kind by name; r and a as the library reads them, from floats)"""
    d = np.asarray(d, np.float64)
    if kind == "box":
        return ((-r <= d) & (d < r)).astype(np.float64)
    if kind == "tent":
        return np.maximum(0.0, 1.0 - np.abs(d) / r)
    if kind == "gaussian":
        return np.where(np.abs(d) < r, np.exp(-a * (d * d)) - math.exp(-a * (r * r)), 0.0)
    x = np.abs(2.0 * d / r)
    near = ((7.0 * x - 12.0) * x * x + 16.0 / 3.0) / 6.0
    far = (((-7.0 / 3.0 * x + 12.0) * x - 20.0) * x + 32.0 / 3.0) / 6.0
    return np.where(np.abs(d) < r, np.where(x < 1.0, near, far), 0.0)


def gather(frame, wx, wy):
    """one pass through its weight tables: (S, W, A) with S = sum w c and A = sum |w c| over the in-frame taps of
    non-zero weight in row-major tap order (j outer, i inner), W = sum w; S and A (h, w, 3), W (h, w)"""
    c = np.asarray(frame, np.float64)
    h, w = c.shape[:2]
    S, A, W = np.full(c.shape, -0.0), np.zeros(c.shape), np.full((h, w), -0.0)
    for j in range(TAPS):
        for i in range(TAPS):
            wt = float(wx[i]) * float(wy[j])
            if wt == 0.0:
                continue
            dx, dy = i - 2, j - 2
            # output pixels p whose tap p + (dx, dy) lies in the frame
            x0, x1, y0, y1 = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
            if x0 >= x1 or y0 >= y1:
                continue
            t = wt * c[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            S[y0:y1, x0:x1] += t
            A[y0:y1, x0:x1] += np.abs(t)
            W[y0:y1, x0:x1] += wt
    return S, W, A


def fold(frames, weights):
    """the filtered fold over the pass frames, in order: (mean, m2, wsum, A) with A = max_k sum |w c| / W_k"""
    mean = m2 = wsum = amp = None
    for k, (x, (wx, wy)) in enumerate(zip(frames, weights)):
        S, W, A = gather(x, wx, wy)
        assert np.all(W > 0)
        Wk = W[..., None]
        with np.errstate(invalid="ignore", over="ignore"):
            f = S / Wk
            if k == 0:
                mean, m2, wsum, amp = f, np.zeros(f.shape), Wk.copy(), A / Wk
                continue
            wsum = wsum + Wk
            d = f - mean
            mean = mean + (d * Wk) / wsum
            m2 = m2 + (Wk * d) * (f - mean)
            amp = np.maximum(amp, A / Wk)
    return mean, m2, wsum, amp


def variance_of(m2, wsum, n):
    return m2 / (wsum * (n - 1)) if n > 1 else np.zeros(m2.shape)


def error_of(mean, var, n):
    """E = sqrt(sum var) / sum |mean| over the pixels with a finite mean, in float64"""
    if n < 2:
        return 0.0
    ok = np.isfinite(mean).all(axis=-1)
    den = np.abs(mean[ok]).sum()
    return float(np.sqrt(var[ok].sum()) / den) if den else 0.0


def reconstruct(fine, s, kind, r, a=2.0):
    """the (h, w, 3) frame whose pixel p is the filter's weighted mean of the s x s supersampled frame's samples
    (fine sample column c sits at pixel coordinate (c - (s-1)/2) / s; the samples outside the frame are missing
    and the weights renormalised, as the fold does at the border)"""
    fine = np.asarray(fine, np.float64)
    H, W = fine.shape[:2]
    h, w = H // s, W // s

    def table(n_fine, n):
        pos = (np.arange(n_fine) - (s - 1) / 2.0) / s
        return f_eval(kind, pos[None, :] - np.arange(n)[:, None], r, a)  # (n, n_fine)

    wx, wy = table(W, w), table(H, h)
    rows = np.tensordot(wy, fine, axes=(1, 0))  # (h, W, 3)
    num = np.tensordot(wx, rows, axes=(1, 1)).transpose(1, 0, 2)  # (h, w, 3)
    den = np.outer(wy.sum(axis=1), wx.sum(axis=1))
    return num / den[..., None]
