"""Progressive accumulation restated with numpy (rtggx_set_accumulation, include/rtggx.h; DESIGN.md "Progressive accumulation").

The device adds every frame's unpacked RayTracingOut0 / RayTracingOut1 words to two running sums of four floats per pixel -- sum r, sum g,
sum b, sum Y^2 with Y = (0.25 r + 0.5 g) + 0.25 b -- in fp32, one operation at a time, in frame order.  numpy's float32 arithmetic is the
same IEEE arithmetic (no contraction between two ufuncs), so the sums can be restated bit for bit: Accumulator below takes the frames'
words, the visibility words and the two instances' metallic, and keeps the sums the device must hold.  converged() is
rtggx_present_accumulation's image, mean_variance() the float64 figures a user derives from the sums."""
import numpy as np


def unpack_r11g11b10f(words):
    """R11G11B10_FLOAT -> float32 [..., 3], exact (every value of the format is a float32), non-finite codes as the device builds them:
    exponent 31 becomes the float32 exponent 255 with the mantissa bits shifted up."""
    w = np.asarray(words, np.uint32)

    def uf(v, mb):
        e, m = v >> np.uint32(mb), v & np.uint32((1 << mb) - 1)
        den = m.astype(np.float32) * np.float32(2.0 ** (-14 - mb))
        bits = np.where(e == 31, np.uint32(0x7F800000), (e + np.uint32(112)) << np.uint32(23)) | (m << np.uint32(23 - mb))
        return np.where(e == 0, den, bits.astype(np.uint32).view(np.float32))
    return np.stack([uf(w & np.uint32(0x7FF), 6), uf((w >> np.uint32(11)) & np.uint32(0x7FF), 6), uf(w >> np.uint32(22), 5)], axis=-1)


def luma(rgb):
    """(0.25 r + 0.5 g) + 0.25 b in float32: the Y of the temporal pass's YCoCg."""
    rgb = np.asarray(rgb, np.float32)
    return (np.float32(0.25) * rgb[..., 0] + np.float32(0.5) * rgb[..., 1]) + np.float32(0.25) * rgb[..., 2]


def diffuse_mask(visibility, metallic):
    """Where a frame writes RayTracingOut1: covered pixels whose instance's metallic is below 1 (resolveSamplesKernel's diffMask rule)."""
    vis = np.asarray(visibility, np.uint32)
    inst = (vis - np.uint32(1)) >> np.uint32(24)
    below = np.array([np.float32(metallic[0]) < 1.0, np.float32(metallic[1]) < 1.0])
    return (vis != 0) & (inst < 2) & below[np.minimum(inst, 1)]


def same_bits(a, b):
    """Element-wise: the same float32 bits, or both NaN (a NaN's payload is the adder's business)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


class Accumulator:
    """The sums of a context of height x width pixels rendering rows [row_begin, row_end): RTGGX_BUF_ACC_REFL / _DIFF and the count."""

    def __init__(self, height, width, row_begin=0, row_end=None):
        self.rows = slice(row_begin, height if row_end is None else row_end)
        self.refl = np.zeros((height, width, 4), np.float32)
        self.diff = np.zeros((height, width, 4), np.float32)
        self.frames = 0

    def reset(self):
        self.refl[...] = 0; self.diff[...] = 0; self.frames = 0

    @staticmethod
    def _add(acc, words, mask):
        rgb = unpack_r11g11b10f(words)
        y = luma(rgb)
        with np.errstate(invalid="ignore", over="ignore"):
            new = acc + np.concatenate([rgb, (y * y)[..., None]], axis=-1)      # one float32 addition per component
        acc[mask] = new[mask]

    def add(self, refl_words, diff_words, visibility, metallic):
        r = self.rows
        own = np.ones(np.asarray(refl_words)[r].shape, bool)
        self._add(self.refl[r], np.asarray(refl_words)[r], own)
        self._add(self.diff[r], np.asarray(diff_words)[r], diffuse_mask(np.asarray(visibility)[r], metallic))
        self.frames += 1

    def converged(self):
        """RTGGX_BUF_CONVERGED as uint64 [H, W]: per component (float)((double)sum / n) of each image, added in float32, alpha 1, RGBA16F."""
        n = np.float64(self.frames)
        with np.errstate(invalid="ignore", over="ignore"):
            m = (self.refl[..., :3].astype(np.float64) / n).astype(np.float32) + (self.diff[..., :3].astype(np.float64) / n).astype(np.float32)
            half = np.concatenate([m, np.ones(m.shape[:-1] + (1,), np.float32)], axis=-1).astype(np.float16)
        return np.ascontiguousarray(half).view(np.uint64)[..., 0]


def mean_variance(sums, frames):
    """From one image's sums [H, W, 4] and the frame count, in float64: (mean rgb [H, W, 3], variance of Y [H, W]) --
    variance = sum Y^2 / n - (mean Y)^2 with mean Y = 0.25 mean r + 0.5 mean g + 0.25 mean b (the population variance; not clamped)."""
    s = np.asarray(sums, np.float64)
    mean = s[..., :3] / frames
    my = 0.25 * mean[..., 0] + 0.5 * mean[..., 1] + 0.25 * mean[..., 2]
    return mean, s[..., 3] / frames - my * my
