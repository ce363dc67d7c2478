"""Scoring against a reference restated with numpy (rtggx_set_scoring, include/rtggx.h; DESIGN.md "Scoring against a reference").

The device reduces, per frame, nine float64 sums and three counts over the pixels of the context's own rows.  Every per-pixel term is a
handful of float64 operations on values that are exact in float64 (halves, 11- and 10-bit floats), and the order of every sum is fixed by
the contract: the terms of pixels p = 0 .. P - 1, row-major from row_begin, padded with +0.0 to the next power of two and added pairwise,
adjacent pairs first.  numpy's float64 arithmetic is the same IEEE arithmetic, one rounding per ufunc, so the record can be restated bit
for bit.  score() takes the words read back from a context -- TemporalSSOut[parity], both raw images, visibility --, the two instances'
metallic and the reference's words, and returns the record the device must have written.  It shares nothing with the kernels but the
contract: no chunk, no lane, no stage."""
import math

import numpy as np

import accum_ref as AR

SUMS = ("se_out_rgb", "se_out_luma", "se_raw_rgb", "se_raw_luma", "ref_rgb2", "ref_luma2", "se_out_rgb_cov", "se_raw_rgb_cov", "ref_rgb2_cov")
COUNTS = ("pixels", "covered", "skipped_out", "skipped_raw")


def tree_sum(x):
    """The contract's sum: x padded with +0.0 to the next power of two, then x[2 i] + x[2 i + 1] level by level.  Empty: +0.0."""
    x = np.asarray(x, np.float64).reshape(-1)
    if x.size == 0:
        return 0.0
    n = 1 << (x.size - 1).bit_length()
    x = np.concatenate([x, np.zeros(n - x.size, np.float64)])
    with np.errstate(invalid="ignore", over="ignore"):
        while len(x) > 1:
            x = x[0::2] + x[1::2]
    return float(x[0])


def tree_levels(count):
    """ceil(log2 P): the additions on the path from any term to the root."""
    return 0 if count <= 1 else (count - 1).bit_length()


def tree_bound(x):
    """|tree_sum(x) - the exact sum| <= ceil(log2 P) 2^-53 sum |x| for non-negative finite x: each level rounds once, by at most 2^-53 of
    the partial sum it forms (half an ulp of a value is at most 2^-53 of it), and the partial sums of one level add up to at most
    sum |x| (1 + 2^-53)^level -- the second-order terms are below 2^-100 of the sum at any P a frame can have and are left out."""
    x = np.asarray(x, np.float64).reshape(-1)
    return tree_levels(x.size) * 2.0 ** -53 * math.fsum(np.abs(x))


def unpack_rgba16f(words):
    """uint64 RGBA16F words -> float64 [..., 3] rgb, exact."""
    w = np.ascontiguousarray(words, np.uint64)
    return w.view(np.float16).reshape(w.shape + (4,))[..., :3].astype(np.float64)


def _luma(c):
    return (0.25 * c[..., 0] + 0.5 * c[..., 1]) + 0.25 * c[..., 2]


def _energy(c):
    return (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]


def terms(tss, refl, diff, visibility, metallic, reference, row_begin=0, row_end=None):
    """The per-pixel terms of the context's own rows, each a float64 vector of P values in pixel order (dict by SUMS), and the counts."""
    rows = slice(row_begin, np.asarray(tss).shape[0] if row_end is None else row_end)
    out = unpack_rgba16f(np.asarray(tss)[rows]).reshape(-1, 3)
    ref = unpack_rgba16f(np.asarray(reference)[rows]).reshape(-1, 3)
    vis = np.asarray(visibility, np.uint32)[rows].reshape(-1)
    covered = vis != 0
    dmask = AR.diffuse_mask(vis, metallic)
    raw = AR.unpack_r11g11b10f(np.asarray(refl)[rows].reshape(-1)).astype(np.float64)
    d1 = AR.unpack_r11g11b10f(np.asarray(diff)[rows].reshape(-1)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        raw = np.where(dmask[:, None], raw + d1, raw)
        ref_ok = np.isfinite(ref).all(axis=-1)
        out_ok = ref_ok & np.isfinite(out).all(axis=-1)
        raw_ok = ref_ok & np.isfinite(raw).all(axis=-1)
        y_ref = _luma(ref)
        zero = np.zeros(len(vis), np.float64)
        t = {
            "se_out_rgb": np.where(out_ok, _energy(out - ref), zero),
            "se_out_luma": np.where(out_ok, (_luma(out) - y_ref) * (_luma(out) - y_ref), zero),
            "se_raw_rgb": np.where(raw_ok, _energy(raw - ref), zero),
            "se_raw_luma": np.where(raw_ok, (_luma(raw) - y_ref) * (_luma(raw) - y_ref), zero),
            "ref_rgb2": np.where(out_ok, _energy(ref), zero),
            "ref_luma2": np.where(out_ok, y_ref * y_ref, zero),
        }
    t["se_out_rgb_cov"] = np.where(covered, t["se_out_rgb"], zero)
    t["se_raw_rgb_cov"] = np.where(covered, t["se_raw_rgb"], zero)
    t["ref_rgb2_cov"] = np.where(covered, t["ref_rgb2"], zero)
    counts = {"pixels": int(len(vis)), "covered": int(covered.sum()), "skipped_out": int((~out_ok).sum()), "skipped_raw": int((~raw_ok).sum())}
    return t, counts


def score(tss, refl, diff, visibility, metallic, reference, row_begin=0, row_end=None):
    """The record (without index and frame_index): the counts, and every sum in the contract's order."""
    t, counts = terms(tss, refl, diff, visibility, metallic, reference, row_begin, row_end)
    rec = dict(counts)
    for k in SUMS:
        rec[k] = tree_sum(t[k])
    return rec


def same_record(got, want):
    """Names of the fields of `want` that `got` does not hold bit for bit (sums by their float64 bits)."""
    bad = [k for k in COUNTS if k in want and int(got[k]) != int(want[k])]
    bad += [k for k in SUMS if np.float64(got[k]).view(np.uint64) != np.float64(want[k]).view(np.uint64)]
    return bad


def figures(rec):
    """What -score writes per frame: sqrt(se / ref2), None where the reference's energy is 0."""
    def rel(se, ref2):
        return math.sqrt(rec[se] / rec[ref2]) if rec[ref2] > 0.0 and math.isfinite(rec[se]) else None
    return {"rel_l2_out": rel("se_out_rgb", "ref_rgb2"), "rel_l2_raw": rel("se_raw_rgb", "ref_rgb2"),
            "rel_l2_out_cov": rel("se_out_rgb_cov", "ref_rgb2_cov"), "rel_l2_raw_cov": rel("se_raw_rgb_cov", "ref_rgb2_cov"),
            "rel_l2_out_luma": rel("se_out_luma", "ref_luma2"), "rel_l2_raw_luma": rel("se_raw_luma", "ref_luma2")}
