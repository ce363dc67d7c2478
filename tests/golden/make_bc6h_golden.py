"""Writes tests/golden/bc6h_pillow.npz: BC6H blocks and what Pillow's DDS plugin decodes them to (8-bit RGB).  Pillow's block decoder is
compiled code that shares no text with this project; it is the witness of the layout table in tests/bc6h_cases.py, of the oracle
(oracle/orc_dds.h) and, through them, of the kernel.  Only this script imports PIL; the tests read the committed file
(tests/test_bc6h_host.py).  Run it from the repository root with a Pillow that reads BC6H (10.1 or later; the committed file: see its
"pillow_version"):  python tests/golden/make_bc6h_golden.py

Each block travels as a one-level DX10 2D DDS file built in memory (128-byte header, then format, 3, 0, 1, 0), once alone in a 4 x 4 image
and once among many in a wide image; both must give the same texels.

UF16 (format 95): every mode, random blocks and crafted ones whose values land mostly in [1/8, 1], where 8 bits still see a 10-bit
endpoint's last bit.  SF16 (format 96): modes 0x1e, 0x03 and 0x0f the same way; for the nine transformed modes below 16 bits only blocks
whose endpoints are all non-negative after the transform with no wrap ("tame" below) -- outside them Pillow saturates where the rules give
a small value, which fits a decoder that does not sign-extend (w + delta) again after masking it.  Whether Pillow agrees with the model on
the tame blocks is measured here; a mode where it does not is left out and named in "sf16_left_out".

Pillow's rounding: its interpolation turns out to lack the format's rounding term (v = (a (64 - w) + b w + 32) >> 6 without the 32): with
the term left out, the model of bc6h_cases.py equals Pillow on every channel stored here, which main() asserts.  In the modes whose
endpoints are wider than 10 bits that puts Pillow one 8-bit step below the format on about 2 % of the channels that lie in (0, 1): half of
the sums change, 31/64 of those move the half by one step, and a half's step is 1/8 ... 1/32 of an 8-bit step in [1/8, 1).  "kind_<fmt>"
says which stored blocks are crafted (0), wrapping (1) or random (2), because the share of such channels depends on it.

Bit sensitivity: for every mode, format and block position p after the mode bits the script looks, among the first TRIES stored blocks B of that mode, for one with Pillow(B) != Pillow(B ^ (1 << p)); "witnessed_<fmt>" holds, per mode, the 128-bit mask of the positions found (as 16
bytes, little endian).  Where B ^ (1 << p) is itself a block Pillow can be trusted on, it is stored too, so that the tests compare the models
with Pillow on both sides of the flip."""
import io
import os
import struct
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bc6h_cases as BC  # noqa: E402

UF16, SF16 = 95, 96
N_RANDOM, N_CRAFTED, N_WRAP, TRIES = 64, 40, 8, 64
SF16_FULL = (0x1e, 0x03, 0x0f)


def dds(blocks, fmt, bw, bh):
    assert blocks.shape == (bw * bh, 16)
    pf = struct.pack("<II4sIIIII", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    head = struct.pack("<4sIIIIIII", b"DDS ", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, 4 * bh, 4 * bw, 16 * bw * bh, 0, 1) + bytes(44) + pf + struct.pack("<IIIII", 0x1000, 0, 0, 0, 0)
    assert len(head) == 128
    return head + struct.pack("<IIIII", fmt, 3, 0, 1, 0) + blocks.tobytes()


def pillow(blocks, fmt, per_image=64):
    """uint8 [n, 16] -> uint8 [n, 16, 3], up to per_image blocks side by side in one image."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    out = np.zeros((len(blocks), 16, 3), np.uint8)
    for at in range(0, len(blocks), per_image):
        part = blocks[at:at + per_image]
        im = Image.open(io.BytesIO(dds(part, fmt, len(part), 1)))
        px = np.asarray(im.convert("RGB"))
        assert px.shape == (4, 4 * len(part), 3) and im.mode == "RGB", (px.shape, im.mode)
        out[at:at + len(part)] = px.reshape(4, len(part), 4, 3).transpose(1, 0, 2, 3).reshape(len(part), 16, 3)
    return out


def tame(block):
    """SF16: every endpoint that the block uses is non-negative, and no (w + delta) leaves [0, 2^(b-1) - 1]."""
    mid, fields, _, _ = BC.parse(block)
    md = BC.MODES[mid]
    for c, ch in enumerate("rgb"):
        w = fields[ch + "w"]
        if w >> (md.wbits - 1):
            return False
        for name in ("x", "y", "z") if md.regions == 2 else ("x",):
            v = w + BC.sign_extend(fields[ch + name], md.delta[c]) if md.transformed else BC.sign_extend(fields[ch + name], md.wbits)
            if not 0 <= v < (1 << (md.wbits - 1)):
                return False
    return True


def trusted(block, fmt):
    return fmt == UF16 or BC.mode_of(block) in SF16_FULL or tame(block)


def crafted(rng, mid, fmt, n):
    """Blocks whose endpoints sit where a half is mostly in [1/8, 1]: 0.387 ... 0.484 of the (positive) endpoint range."""
    md, out = BC.MODES[mid], []
    span = 1 << (md.wbits if fmt == UF16 else md.wbits - 1)
    lo, hi = int(0.387 * span), max(int(0.484 * span), int(0.387 * span) + 1)
    while len(out) < n:
        d = int(rng.integers(0, 32))
        fields = {}
        for c, ch in enumerate("rgb"):
            fields[ch + "w"] = int(rng.integers(lo, hi + 1))
            for name in "xyz":
                fields[ch + name] = int(rng.integers(0, 1 << md.delta[c])) if md.transformed else int(rng.integers(max(lo - span // 8, 0), min(hi + span // 16, span - 1) + 1))
        widths = BC.index_layout(md, d)[1]
        blk = np.frombuffer(BC.assemble(mid, fields, d, [int(rng.integers(0, 1 << w)) for w in widths]), np.uint8)
        if trusted(blk, fmt):
            out.append(blk)
    return np.stack(out)


def wrapping(rng, mid, fmt, n):
    """One-region transformed modes: a delta that wraps through the endpoint width, so that the two endpoints are far apart (a 4-bit delta
    alone moves a 16-bit endpoint by less than 8 bits can see).  UF16: w just above 0, the delta reaching below it.  SF16: w just below
    2^(b-1), the delta reaching above it.  Indices 4 and 5: of the 16 interpolated values only those of indices 4 ... 7 (UF16) or 4, 5 (SF16)
    fall into (1/255, 1), and from 4 or 5 a flip of any of the four index bits changes what 8 bits show."""
    md, out = BC.MODES[mid], []
    for _ in range(n):
        fields = {}
        for c, ch in enumerate("rgb"):
            k = int(rng.integers(1, 1 << (md.delta[c] - 2)))
            if fmt == UF16:
                fields[ch + "w"], fields[ch + "x"] = k, int(rng.integers(-(1 << (md.delta[c] - 1)), -k)) & ((1 << md.delta[c]) - 1)
            else:
                fields[ch + "w"], fields[ch + "x"] = (1 << (md.wbits - 1)) - 1 - k, int(rng.integers(k + 1, 1 << (md.delta[c] - 1)))
        out.append(np.frombuffer(BC.assemble(mid, fields, 0, [int(v) for v in rng.integers(4, 6, 16)]), np.uint8))
    return np.stack(out) if out else np.zeros((0, 16), np.uint8)


def tame_random(rng, mid, n):
    out = []
    while len(out) < n:
        blk = BC.random_blocks(rng, mid, 1)[0]
        md = BC.MODES[mid]
        mid_, fields, d, idx = BC.parse(blk)
        for c, ch in enumerate("rgb"):                       # pull w into the positive half, and not too near its ends, so that random deltas often stay inside
            fields[ch + "w"] = int(rng.integers(0, 1 << (md.wbits - 1)))
        blk = np.frombuffer(BC.assemble(mid, fields, d, idx), np.uint8)
        if tame(blk):
            out.append(blk)
    return np.stack(out)


def main():
    rng = np.random.default_rng(0x6BC)
    store = {}
    for fmt, key in ((UF16, "uf16"), (SF16, "sf16")):
        blocks, kinds, left_out = [], [], []
        for mid in BC.MODE_IDS:
            if fmt == UF16 or mid in SF16_FULL:
                wrap = BC.MODES[mid].transformed and BC.MODES[mid].regions == 1
                own = np.concatenate([crafted(rng, mid, fmt, N_CRAFTED), wrapping(rng, mid, fmt, N_WRAP if wrap else 0), BC.random_blocks(rng, mid, N_RANDOM)])
                kind = [0] * N_CRAFTED + [1] * (N_WRAP if wrap else 0) + [2] * N_RANDOM
            else:
                own = np.concatenate([crafted(rng, mid, fmt, N_CRAFTED), tame_random(rng, mid, N_RANDOM)])
                kind = [0] * N_CRAFTED + [2] * N_RANDOM
                ours = BC.half_to_8bit(BC.decode_blocks(own, True))
                diff = np.abs(pillow(own, fmt).astype(int) - ours.astype(int))
                print("SF16 mode %#04x tame blocks: Pillow within %d of the model, %d of %d channels differ" % (mid, diff.max(), (diff > 0).sum(), diff.size))
                if diff.max() > 1:
                    left_out.append(mid)
                    continue
            blocks.append(own)
            kinds += kind
        blocks = np.concatenate(blocks)
        texels = pillow(blocks, fmt)
        # bit sensitivity
        modes = np.array([BC.mode_of(b) for b in blocks])
        masks, flips = np.zeros((len(BC.MODE_IDS), 16), np.uint8), []          # flips: (index of B, p)
        for mi, mid in enumerate(BC.MODE_IDS):
            at = np.nonzero(modes == mid)[0][:TRIES]                      # the crafted ones come first
            if at.size == 0:
                continue
            mask = 0
            for p in range(BC.MODES[mid].mode_bits, 128):
                flipped = blocks[at].copy()
                flipped[:, p >> 3] ^= 1 << (p & 7)
                seen = (pillow(flipped, fmt) != texels[at]).any(axis=(1, 2))
                if not seen.any():
                    continue
                mask |= 1 << p
                ok = [k for k in np.nonzero(seen)[0] if trusted(flipped[k], fmt)]
                if ok:
                    flips.append((at[ok[0]], p))
            masks[mi] = np.frombuffer(mask.to_bytes(16, "little"), np.uint8)
            missing = [p for p in range(BC.MODES[mid].mode_bits, 128) if not (mask >> p) & 1]
            print("%s mode %#04x: %d positions witnessed, not witnessed: %s" % (key, mid, bin(mask).count("1"), missing))
        flips = np.array(flips)
        flipped = blocks[flips[:, 0]].copy()
        flipped[np.arange(len(flips)), flips[:, 1] >> 3] ^= (1 << (flips[:, 1] & 7)).astype(np.uint8)
        flip_texels = pillow(flipped, fmt)
        # one block per image gives the same texels as many per image
        alone = np.concatenate([pillow(b, fmt, per_image=1) for b in np.concatenate([blocks, flipped])])
        assert np.array_equal(alone, np.concatenate([texels, flip_texels])), "%s: a block decodes differently alone and among others" % key
        store["blocks_" + key], store["pillow_" + key], store["witnessed_" + key] = blocks, texels, masks
        store["kind_" + key] = np.array(kinds, np.uint8)
        assert len(kinds) == len(blocks)
        for b, t in ((blocks, texels), (flipped, flip_texels)):
            assert np.array_equal(BC.half_to_8bit(BC.decode_blocks(b, fmt == SF16, rounding=0)), t), "%s: Pillow is not the model without the rounding term" % key
        store["flip_base_" + key], store["flip_pos_" + key], store["pillow_flip_" + key] = flips[:, 0].astype(np.uint16), flips[:, 1].astype(np.uint8), flip_texels
        store[key + "_left_out"] = np.array(left_out, np.int32)
        print("%s: %d blocks and %d flips" % (key, len(blocks), len(flips)))
    store["formats"] = np.array([UF16, SF16], np.int32)
    store["mode_ids"] = np.array(BC.MODE_IDS, np.int32)
    store["pillow_version"] = np.array(PIL.__version__)
    path = os.path.join(HERE, "bc6h_pillow.npz")
    np.savez_compressed(path, **store)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
