"""numpy restatement of the clipped step -- TEST INFRASTRUCTURE ONLY.

``adam_factors_clip`` is ``oracle.adam_factors`` with g = (raw x F32(1e16)) x F32(coef): the clip is a
float32 multiply of its own in front of Adam's sequence.  test_clip_host.py pins it to the oracle bit for
bit at coef = 1.  ``clip_record`` is the arithmetic of the device's finish step in numpy.
"""
import numpy as np

F32 = np.float32


def adam_factors_clip(grad_raw, m, v, t, lr, coef, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1e16):
    g = (np.asarray(grad_raw, F32) * F32(grad_scale)) * F32(coef)
    m_new = F32(beta1) * np.asarray(m, F32) + F32(1 - beta1) * g
    v_new = F32(beta2) * np.asarray(v, F32) + F32(1 - beta2) * (g * g)
    m_hat = m_new / F32(1 - beta1 ** t)
    v_hat = v_new / F32(1 - beta2 ** t)
    delta = F32(lr) * m_hat / (np.sqrt(v_hat) + F32(eps))
    return m_new.astype(F32), v_new.astype(F32), delta.astype(F32)


def sumsq(grad_raw, grad_scale=1e16) -> float:
    """sum double(float32(g x grad_scale))^2 in numpy's (pairwise) float64 order."""
    gs = (np.asarray(grad_raw, F32).reshape(-1) * F32(grad_scale)).astype(np.float64)
    return float(np.sum(gs * gs))


def norm_of(sumsq_value: float) -> np.float32:
    with np.errstate(invalid="ignore"):
        return F32(np.sqrt(np.float64(sumsq_value)))


def coef_of(norm, max_norm) -> np.float32:
    """min(1.0f, float32(c) / (norm + 1e-6f)) in IEEE float32 (torch.nn.utils.clip_grad_norm_)."""
    with np.errstate(over="ignore", divide="ignore"):
        q = F32(max_norm) / (F32(norm) + F32(1e-6))
    return F32(min(F32(1.0), q))


def clip_record(sums, max_norm, skipped_total=0) -> dict:
    """The record of sum(sums) added in index order."""
    s = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in np.asarray(sums, np.float64).reshape(-1):
            s = s + x
    skip = not np.isfinite(s)
    n = norm_of(s)
    return {"sumsq": float(s), "norm": float(n), "coef": 1.0 if skip else float(coef_of(n, max_norm)),
            "skipped": bool(skip), "skipped_total": skipped_total + int(skip)}


def sumsq_bound(n: int) -> float:
    """Worst-case relative error of ANY order of summing n non-negative float64 terms (each square is
    rounded once, each of the n - 1 additions once: (1 + u)^n - 1 <= n 2^-52 for the sizes used)."""
    return max(n, 1) * 2.0 ** -52
