"""Arrays as the tests compare them (test infrastructure): the uint32 words of float
data, the RMS colour difference of two frames, and numpy arrays on the device with a
sentinel tail that no kernel may touch.  What belongs here reads or holds arrays and knows
nothing of scenes or renders (those are in parity_util)."""
import numpy as np


def u32(a):
    """The words of `a` as float32 (converted if need be): compare floats bit for bit."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits(a):
    """The words of a 4-byte array as they are, without conversion."""
    return np.ascontiguousarray(a).view(np.uint32)


def rms(a, b, mask=None):
    """RMS difference of the colour channels, in float64, over the pixels of `mask` or all."""
    d = (a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask])))


class Dev:
    """numpy arrays on the device, with a sentinel tail that must survive"""

    SENTINEL = 0xA5A5A5A5

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        b = self.ctx.alloc(max(16, arr.nbytes))
        if arr.nbytes:
            b.from_numpy(arr)
        self.bufs.append(b)
        return b

    def out(self, nwords, tail=64):
        b = self.ctx.alloc((nwords + tail) * 4)
        b.from_numpy(np.full(nwords + tail, self.SENTINEL, np.uint32))
        self.bufs.append(b)
        return b

    @classmethod
    def get(cls, b, nwords, tail=64):
        a = b.to_numpy(np.uint32, (nwords + tail,))
        over = np.flatnonzero(a[nwords:] != cls.SENTINEL)
        assert over.size == 0, (f"{over.size} of the {tail} words behind a buffer of {nwords} were written, "
                                f"first at +{over[:4].tolist()}: {[hex(x) for x in a[nwords:][over[:4]]]}")
        return a[:nwords]

    def close(self):
        for b in self.bufs:
            b.free()
