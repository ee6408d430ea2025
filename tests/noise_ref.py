"""numpy float32 restatement of the noise estimate, written from the definition in
include/rt.h ("noise estimate") alone (test infrastructure; independent of the kernels).
Every line is one IEEE f32 operation on whole arrays -- numpy fuses nothing, and its f32
division and square root are correctly rounded -- so the GPU state, map and summary are
held to these bit for bit.

    y = (0.2126f*x.x + 0.7152f*x.y) + 0.0722f*x.z
    n = (float)(it + 1)
    d = y - mean;  mean = mean + d / n;  m2 = m2 + d * (y - mean)
    rel = sqrtf((m2 < 0 ? 0 : m2) / (nf * (nf - 1.0f))) / max(|mean|, floor)
"""
import numpy as np

f32 = np.float32
WR, WG, WB = f32(0.2126), f32(0.7152), f32(0.0722)
QNAN_BITS = 0x7FC00000


def luminance(records):
    """records float32[..., >= 3] -> y float32[...]"""
    r = np.asarray(records, dtype=f32)
    with np.errstate(all="ignore"):
        return (WR * r[..., 0] + WG * r[..., 1]) + WB * r[..., 2]


def accumulate_y(y, first_iter=0, state=None):
    """y float32[npix, spp]: the luminance of iterations first_iter.. in order, folded into
    state float32[npix, 2] ({mean, m2}; None or first_iter == 0: {0, 0}).  Returns the new state."""
    y = np.asarray(y, dtype=f32)
    npix, spp = y.shape
    if first_iter == 0 or state is None:
        mean = np.zeros(npix, f32)
        m2 = np.zeros(npix, f32)
    else:
        mean = np.array(state[:, 0], dtype=f32)
        m2 = np.array(state[:, 1], dtype=f32)
    with np.errstate(all="ignore"):
        for i in range(spp):
            n = f32(first_iter + i + 1)
            d = y[:, i] - mean
            mean = mean + d / n
            m2 = m2 + d * (y[:, i] - mean)
    assert mean.dtype == f32 and m2.dtype == f32
    return np.stack([mean, m2], axis=-1)


def accumulate(records, first_iter=0, state=None):
    """records float32[npix, spp, 4] ([pixel][iteration]; w is not read)"""
    return accumulate_y(luminance(records), first_iter, state)


def nonfinite(state):
    return ~(np.isfinite(state[:, 0]) & np.isfinite(state[:, 1]))


def rel_map(state, n, floor):
    """float32[npix]: rel after n >= 2 iterations; the quiet NaN 0x7FC00000 for a non-finite state."""
    assert n >= 2 and floor > 0
    state = np.asarray(state, dtype=f32)
    mean, m2 = state[:, 0], state[:, 1]
    nf = f32(n)
    denom = nf * (nf - f32(1.0))
    with np.errstate(all="ignore"):
        var = np.where(m2 < 0, f32(0.0), m2) / denom
        a = np.abs(mean)
        rel = np.sqrt(var) / np.where(a < f32(floor), f32(floor), a)
    assert rel.dtype == f32
    bits = rel.view(np.uint32).copy()
    bits[nonfinite(state)] = QNAN_BITS
    return bits.view(f32)


def summary(state, n, threshold, floor):
    """{pixels, above, nonfinite, max_rel_err (float32)} as rt_noise_summarize defines them."""
    rel = rel_map(state, n, floor)
    bad = nonfinite(np.asarray(state, dtype=f32))
    good = rel[~bad]
    return {"pixels": int(rel.size), "above": int((good > f32(threshold)).sum()), "nonfinite": int(bad.sum()),
            "max_rel_err": f32(good.max()) if good.size else f32(0.0)}
