"""BC6H blocks with known answers: a field assembler with its own bit-layout table, an exact-integer model of the decode written from
the format's rules, and the deterministic cases the host and GPU tests share (tests/test_bc6h_host.py, tests/test_gpu_bc6h.py).

Nothing here calls the oracle (oracle/orc_dds.h) or reads the kernel (raytracedggx_amd/csrc/env.hip).  Both of those keep their layouts as
one string per mode in STREAM order (for each position of the block, the field bit that sits there).  The table below is FIELD-major (for
each bit of each field, its position in the block) and was written down field by field; the partitions are 16-bit masks, not rows.  A
transcription slip in one notation does not reproduce in the other.  What witnesses this table is not its author but a decoder that shares
no text with the project: tests/golden/bc6h_pillow.npz (tests/golden/make_bc6h_golden.py).

The rules (Direct3D 11 "BC6H format"; Khronos Data Format Specification, "BPTC float"), with endpoints w (region 0, first), x (region 0,
second), y and z (region 1) per channel, b = the mode's endpoint width and d_c the channel's delta width:
  transform   x, y, z are d_c-bit two's-complement deltas: e = (w + delta) mod 2^b            (every mode but 0x1e and 0x03)
  SF16        each endpoint is then read as a b-bit two's-complement number
  unquantize  UF16: b >= 15: e;  e = 0: 0;  e = 2^b - 1: 0xFFFF;  else ((e << 16) + 0x8000) >> b
              SF16: b >= 16: e;  on |e|:  0: 0;  |e| >= 2^(b-1) - 1: 0x7FFF;  else ((|e| << 15) + 0x4000) >> (b - 1);  the sign put back
  regions     two-region modes: texel i belongs to region (PARTITION[d] >> i) & 1
  indices     3 bits per texel with two regions, 4 with one; texel 0 and, with two regions, texel ANCHOR[d] store one bit less (the top bit is 0)
  interpolate v = (a (64 - wt) + b wt + 32) >> 6, the shift rounding toward minus infinity
  finish      UF16: (v * 31) >> 6;  SF16: (|v| * 31) >> 5 with bit 15 set where v < 0        -> a binary16 bit pattern
The four five-bit ids 0x13, 0x17, 0x1b and 0x1f are reserved and decode to zeros."""
import functools
from collections import namedtuple

import numpy as np

FIELDS = ("rw", "rx", "ry", "rz", "gw", "gx", "gy", "gz", "bw", "bx", "by", "bz")
Mode = namedtuple("Mode", "id mode_bits transformed regions wbits delta pos")


def _r(lo, hi):
    return list(range(lo, hi + 1))


def _mode(mid, transformed, regions, wbits, delta, **pos):
    pos.setdefault("d", _r(77, 81) if regions == 2 else [])
    for f in FIELDS:
        pos.setdefault(f, [])
    return Mode(mid, 2 if mid < 2 else 5, transformed, regions, wbits, delta, pos)


# pos[field][k] = position in the block of bit k of the field
MODES = {m.id: m for m in (
    _mode(0x00, 1, 2, 10, (5, 5, 5), rw=_r(5, 14), gw=_r(15, 24), bw=_r(25, 34), rx=_r(35, 39), gx=_r(45, 49), bx=_r(55, 59),
          ry=_r(65, 69), gy=_r(41, 44) + [2], by=_r(61, 64) + [3], rz=_r(71, 75), gz=_r(51, 54) + [40], bz=[50, 60, 70, 76, 4]),
    _mode(0x01, 1, 2, 7, (6, 6, 6), rw=_r(5, 11), gw=_r(15, 21), bw=_r(25, 31), rx=_r(35, 40), gx=_r(45, 50), bx=_r(55, 60),
          ry=_r(65, 70), gy=_r(41, 44) + [24, 2], by=_r(61, 64) + [14, 22], rz=_r(71, 76), gz=_r(51, 54) + [3, 4], bz=[12, 13, 23, 32, 34, 33]),
    _mode(0x02, 1, 2, 11, (5, 4, 4), rw=_r(5, 14) + [40], gw=_r(15, 24) + [49], bw=_r(25, 34) + [59], rx=_r(35, 39), gx=_r(45, 48), bx=_r(55, 58),
          ry=_r(65, 69), gy=_r(41, 44), by=_r(61, 64), rz=_r(71, 75), gz=_r(51, 54), bz=[50, 60, 70, 76]),
    _mode(0x06, 1, 2, 11, (4, 5, 4), rw=_r(5, 14) + [39], gw=_r(15, 24) + [50], bw=_r(25, 34) + [59], rx=_r(35, 38), gx=_r(45, 49), bx=_r(55, 58),
          ry=_r(65, 68), gy=_r(41, 44) + [75], by=_r(61, 64), rz=_r(71, 74), gz=_r(51, 54) + [40], bz=[69, 60, 70, 76]),
    _mode(0x0a, 1, 2, 11, (4, 4, 5), rw=_r(5, 14) + [39], gw=_r(15, 24) + [49], bw=_r(25, 34) + [60], rx=_r(35, 38), gx=_r(45, 48), bx=_r(55, 59),
          ry=_r(65, 68), gy=_r(41, 44), by=_r(61, 64) + [40], rz=_r(71, 74), gz=_r(51, 54), bz=[50, 69, 70, 76, 75]),
    _mode(0x0e, 1, 2, 9, (5, 5, 5), rw=_r(5, 13), gw=_r(15, 23), bw=_r(25, 33), rx=_r(35, 39), gx=_r(45, 49), bx=_r(55, 59),
          ry=_r(65, 69), gy=_r(41, 44) + [24], by=_r(61, 64) + [14], rz=_r(71, 75), gz=_r(51, 54) + [40], bz=[50, 60, 70, 76, 34]),
    _mode(0x12, 1, 2, 8, (6, 5, 5), rw=_r(5, 12), gw=_r(15, 22), bw=_r(25, 32), rx=_r(35, 40), gx=_r(45, 49), bx=_r(55, 59),
          ry=_r(65, 70), gy=_r(41, 44) + [24], by=_r(61, 64) + [14], rz=_r(71, 76), gz=_r(51, 54) + [13], bz=[50, 60, 23, 33, 34]),
    _mode(0x16, 1, 2, 8, (5, 6, 5), rw=_r(5, 12), gw=_r(15, 22), bw=_r(25, 32), rx=_r(35, 39), gx=_r(45, 50), bx=_r(55, 59),
          ry=_r(65, 69), gy=_r(41, 44) + [24, 23], by=_r(61, 64) + [14], rz=_r(71, 75), gz=_r(51, 54) + [40, 33], bz=[13, 60, 70, 76, 34]),
    _mode(0x1a, 1, 2, 8, (5, 5, 6), rw=_r(5, 12), gw=_r(15, 22), bw=_r(25, 32), rx=_r(35, 39), gx=_r(45, 49), bx=_r(55, 60),
          ry=_r(65, 69), gy=_r(41, 44) + [24], by=_r(61, 64) + [14, 23], rz=_r(71, 75), gz=_r(51, 54) + [40], bz=[50, 13, 70, 76, 34, 33]),
    _mode(0x1e, 0, 2, 6, (6, 6, 6), rw=_r(5, 10), gw=_r(15, 20), bw=_r(25, 30), rx=_r(35, 40), gx=_r(45, 50), bx=_r(55, 60),
          ry=_r(65, 70), gy=_r(41, 44) + [24, 21], by=_r(61, 64) + [14, 22], rz=_r(71, 76), gz=_r(51, 54) + [11, 31], bz=[12, 13, 23, 32, 34, 33]),
    _mode(0x03, 0, 1, 10, (10, 10, 10), rw=_r(5, 14), gw=_r(15, 24), bw=_r(25, 34), rx=_r(35, 44), gx=_r(45, 54), bx=_r(55, 64)),
    _mode(0x07, 1, 1, 11, (9, 9, 9), rw=_r(5, 14) + [44], gw=_r(15, 24) + [54], bw=_r(25, 34) + [64], rx=_r(35, 43), gx=_r(45, 53), bx=_r(55, 63)),
    _mode(0x0b, 1, 1, 12, (8, 8, 8), rw=_r(5, 14) + [44, 43], gw=_r(15, 24) + [54, 53], bw=_r(25, 34) + [64, 63], rx=_r(35, 42), gx=_r(45, 52), bx=_r(55, 62)),
    _mode(0x0f, 1, 1, 16, (4, 4, 4), rw=_r(5, 14) + [44, 43, 42, 41, 40, 39], gw=_r(15, 24) + [54, 53, 52, 51, 50, 49], bw=_r(25, 34) + [64, 63, 62, 61, 60, 59],
          rx=_r(35, 38), gx=_r(45, 48), bx=_r(55, 58)),
)}
MODE_IDS = tuple(MODES)
RESERVED = (0x13, 0x17, 0x1b, 0x1f)

# bit i of PARTITION[d]: the region of texel i (row-major in the 4 x 4 block)
PARTITION = (0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
             0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C)
# the texel of region 1 whose index is stored one bit short
ANCHOR = (15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2)
WEIGHTS = {3: (0, 9, 18, 27, 37, 46, 55, 64), 4: (0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64)}


def index_layout(md, d):
    """-> (first position, [bits of texel i's index])."""
    ib = 3 if md.regions == 2 else 4
    short = {0} | ({ANCHOR[d]} if md.regions == 2 else set())
    return (82 if md.regions == 2 else 65), [ib - 1 if i in short else ib for i in range(16)]


def assemble(mode_id, fields, d=0, indices=(0,) * 16):
    """A mode id, the fields rw..bz (ints, taken modulo their width; missing ones are 0), the partition and 16 indices -> 16 bytes."""
    md = MODES[mode_id]
    acc = mode_id
    for f in FIELDS:
        v = int(fields.get(f, 0))
        for k, p in enumerate(md.pos[f]):
            acc |= ((v >> k) & 1) << p
    for k, p in enumerate(md.pos["d"]):
        acc |= ((d >> k) & 1) << p
    at, widths = index_layout(md, d if md.regions == 2 else 0)
    for i, n in enumerate(widths):
        assert 0 <= indices[i] < (1 << n), "texel %d: index %d does not fit %d bits" % (i, indices[i], n)
        acc |= indices[i] << at
        at += n
    assert at == 128
    return acc.to_bytes(16, "little")


def parse(block):
    """16 bytes -> (mode id or None if reserved, fields, d, indices), by the same table read the other way."""
    acc = int.from_bytes(bytes(block), "little")
    mid = acc & 3 if (acc & 3) < 2 else acc & 31
    if mid not in MODES:
        return None, {}, 0, [0] * 16
    md = MODES[mid]
    fields = {f: sum(((acc >> p) & 1) << k for k, p in enumerate(md.pos[f])) for f in FIELDS}
    d = sum(((acc >> p) & 1) << k for k, p in enumerate(md.pos["d"]))
    at, widths = index_layout(md, d)
    idx = []
    for n in widths:
        idx.append((acc >> at) & ((1 << n) - 1))
        at += n
    return mid, fields, d, idx


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def sign_extend(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def endpoints(mode_id, fields, signed):
    """-> e[region][k][channel]: the endpoints after the transform, as b-bit numbers (two's-complement ones read as such if signed)."""
    md = MODES[mode_id]
    e = [[[0] * 3 for _ in range(2)] for _ in range(2)]
    for c, ch in enumerate("rgb"):
        w = fields[ch + "w"]
        rest = [fields[ch + "x"], fields[ch + "y"], fields[ch + "z"]]
        if md.transformed:
            rest = [(w + sign_extend(v, md.delta[c])) % (1 << md.wbits) for v in rest]
        vals = [w] + rest
        if signed:
            vals = [sign_extend(v, md.wbits) for v in vals]
        e[0][0][c], e[0][1][c], e[1][0][c], e[1][1][c] = vals
    return e


def unquantize(e, bits, signed):
    if not signed:
        if bits >= 15:
            return e
        if e == 0:
            return 0
        if e == (1 << bits) - 1:
            return 0xFFFF
        return ((e << 16) + 0x8000) >> bits
    if bits >= 16:
        return e
    a = abs(e)
    if a == 0:
        u = 0
    elif a >= (1 << (bits - 1)) - 1:
        u = 0x7FFF
    else:
        u = ((a << 15) + 0x4000) >> (bits - 1)
    return -u if e < 0 else u


def finish(v, signed):
    if not signed:
        return (v * 31) >> 6
    return (0x8000 | ((-v * 31) >> 5)) if v < 0 else (v * 31) >> 5


def decode_fields(mode_id, fields, d, indices, signed, rounding=32):
    """-> 16 texels x 3 channels of binary16 bit patterns (Python ints).  rounding: the interpolation's rounding term; the format says 32."""
    md = MODES[mode_id]
    e = endpoints(mode_id, fields, signed)
    u = [[[unquantize(e[r][k][c], md.wbits, signed) for c in range(3)] for k in range(2)] for r in range(2)]
    wt = WEIGHTS[3 if md.regions == 2 else 4]
    out = []
    for i in range(16):
        r = (PARTITION[d] >> i) & 1 if md.regions == 2 else 0
        w = wt[indices[i]]
        out.append([finish((u[r][0][c] * (64 - w) + u[r][1][c] * w + rounding) >> 6, signed) for c in range(3)])   # Python's >> floors
    return out


def decode_block(block, signed, rounding=32):
    """16 bytes -> uint16 [16, 3]."""
    mid, fields, d, idx = parse(block)
    if mid is None:
        return np.zeros((16, 3), np.uint16)
    return np.array(decode_fields(mid, fields, d, idx, signed, rounding), np.uint16)


def decode_blocks(blocks, signed, rounding=32):
    return np.stack([decode_block(b.tobytes(), signed, rounding) for b in np.asarray(blocks, np.uint8).reshape(-1, 16)]) if len(blocks) else np.zeros((0, 16, 3), np.uint16)


def half_to_8bit(h, rule="trunc32"):
    """binary16 bit patterns -> what an 8-bit RGB decoder shows: below 0 -> 0, above 1 -> 255, else by the rule."""
    v = np.asarray(h, np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(invalid="ignore"):
        if rule == "trunc32":
            q = np.floor(np.clip(v, 0, 1) * np.float32(255))
        elif rule == "round32":
            q = np.floor(np.clip(v, 0, 1) * np.float32(255) + np.float32(0.5))
        elif rule == "trunc64":
            q = np.floor(np.clip(v.astype(np.float64), 0, 1) * 255.0)
        elif rule == "round64":
            q = np.floor(np.clip(v.astype(np.float64), 0, 1) * 255.0 + 0.5)
        else:
            raise ValueError(rule)
    q = np.where(np.isnan(v), 0, q)
    return np.where(v < 0, 0, np.where(v > 1, 255, q)).astype(np.uint8)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def fields_from_endpoints(mode_id, e):
    """e[region][k][channel] as b-bit numbers (negative ones allowed) -> the fields that decode to them; in a transformed mode every endpoint
    must lie within the channel's delta range of w, modulo 2^b."""
    md = MODES[mode_id]
    mask = (1 << md.wbits) - 1
    fields = {}
    for c, ch in enumerate("rgb"):
        w = e[0][0][c] & mask
        fields[ch + "w"] = w
        for name, v in (("x", e[0][1][c]), ("y", e[1][0][c]), ("z", e[1][1][c])):
            if md.regions == 1 and name != "x":
                continue
            if md.transformed:
                dv = (v - w) & ((1 << md.delta[c]) - 1)
                assert (w + sign_extend(dv, md.delta[c])) & mask == v & mask, "mode %#x channel %d: %d is out of the delta's reach from %d" % (mode_id, c, v, w)
                fields[ch + name] = dv
            else:
                fields[ch + name] = v & mask
    return fields


def _nidx(md, d, i):
    return 1 << index_layout(md, d)[1][i]


def _spread_indices(md, d, k):
    """Indices that differ from texel to texel; with k running over range(8 or 16) every texel takes every value it can store."""
    return [(i * 5 + k) % _nidx(md, d, i) for i in range(16)]


def _partition_cases(mid):
    """All 32 partitions with the two regions apart as far as the deltas reach, in the three channels in three different ways."""
    md, out = MODES[mid], []
    top = (1 << md.wbits) - 1
    for d in range(32):
        reach = [(1 << (dc - 1)) - 1 for dc in md.delta] if md.transformed else [top // 3] * 3
        base = [top * 2 // 5 + 3 * c for c in range(3)]
        e = [[[base[c] for c in range(3)], [base[c] + 1 + (d + c) % 2 for c in range(3)]],
             [[base[c] + (reach[c] if c != 1 else -reach[c]) for c in range(3)], [base[c] + (reach[c] - 2 if c != 1 else -reach[c] + 1) for c in range(3)]]]
        out.append(("partition %d" % d, assemble(mid, fields_from_endpoints(mid, e), d, _spread_indices(md, d, d))))
    return out


def _endpoint_cases(mid):
    """The special endpoint values of both unquantize rules, and deltas that wrap through the endpoint width in each direction, per channel."""
    md, out = MODES[mid], []
    b = md.wbits
    top, half = (1 << b) - 1, 1 << (b - 1)
    specials = [0, 1, top, top - 1, half, half + 1, half - 1, half - 2, 2, top - 2]       # as b-bit patterns: top = -1, half = -2^(b-1), half + 1 = -(2^(b-1) - 1)
    ds = [3, 17, 18] if md.regions == 2 else [0]
    n = 0
    for j in range(len(specials)):
        for step in (0, 1, -1, "max", "min"):
            w = [specials[(j + 3 * c) % len(specials)] for c in range(3)]
            if md.transformed:
                dl = [{"max": (1 << (dc - 1)) - 1, "min": -(1 << (dc - 1))}.get(step, step) for dc in md.delta]
                e = [[w, [w[c] + dl[c] for c in range(3)]], [[w[c] - dl[c] if step in (1, -1) else w[c] + dl[(c + 1) % 3] // 2 for c in range(3)], [w[c] + (dl[c] if step in (1, -1) else -dl[c] // 2) for c in range(3)]]]
            else:
                o = {0: 0, 1: 1, -1: -1, "max": 4, "min": 7}[step]
                e = [[w, [specials[(j + o + c) % len(specials)] for c in range(3)]], [[specials[(j + o + 2 * c + 1) % len(specials)] for c in range(3)], [specials[(j + 2 * o + c + 5) % len(specials)] for c in range(3)]]]
            d = ds[n % len(ds)]
            out.append(("endpoints %d %s" % (j, step), assemble(mid, fields_from_endpoints(mid, e), d, _spread_indices(md, d, n))))
            n += 1
    if md.transformed:
        # one endpoint at a time through the wrap, the others at rest: up from the top, down from 0, by 1 and by the delta's full reach
        names = ("x", "y", "z") if md.regions == 2 else ("x",)
        for c, ch in enumerate("rgb"):
            hi, lo = (1 << (md.delta[c] - 1)) - 1, -(1 << (md.delta[c] - 1))
            for name in names:
                for w, dv in ((top, 1), (top, hi), (top - hi + 1, hi), (0, -1), (0, lo), (-lo - 1, lo), (half - 1, 1), (half, -1), (half - 1, hi), (half, lo)):
                    fields = {k: 0 for k in FIELDS}
                    for c2, ch2 in enumerate("rgb"):
                        fields[ch2 + "w"] = w if c2 == c else (top * 2 // 5 + c2)
                    fields[ch + name] = dv & ((1 << md.delta[c]) - 1)
                    d = ds[n % len(ds)]
                    out.append(("wrap %s%s %d%+d" % (ch, name, w, dv), assemble(mid, fields, d, _spread_indices(md, d, n))))
                    n += 1
    return out


def _index_cases(mid):
    """Every index value at every texel, the short indices of texel 0 and of the anchors 15, 2 and 8 included."""
    md, out = MODES[mid], []
    top = (1 << md.wbits) - 1
    for d in ((0, 17, 18) if md.regions == 2 else (0,)):
        reach = [min((1 << (dc - 1)) - 1, top // 4) for dc in md.delta]
        base = [top * 2 // 5 + 5 * c for c in range(3)]
        e = [[base, [base[c] + reach[c] for c in range(3)]], [[base[c] - reach[c] for c in range(3)], [base[c] + reach[c] // 2 for c in range(3)]]]
        fields = fields_from_endpoints(mid, e)
        for k in range(8 if md.regions == 2 else 16):
            out.append(("indices d%d +%d" % (d, k), assemble(mid, fields, d, _spread_indices(md, d, k))))
    return out


def random_blocks(rng, mode_id, n):
    """n blocks of random bits with the mode id in the low bits (2 bits for 0x00 and 0x01, else 5)."""
    blocks = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    nb = 2 if mode_id < 2 else 5
    blocks[:, 0] = (blocks[:, 0] & (0xFF ^ ((1 << nb) - 1))) | mode_id
    return blocks


N_RANDOM = 300


@functools.lru_cache(maxsize=None)
def all_cases():
    """-> (names, uint8 [n, 16]).  Seeded; the same on every call and every machine."""
    names, blocks = [], []
    rng = np.random.default_rng(0xBC6)
    for mid in MODE_IDS:
        crafted = (_partition_cases(mid) if MODES[mid].regions == 2 else []) + _endpoint_cases(mid) + _index_cases(mid)
        for name, blk in crafted:
            names.append("mode %#04x %s" % (mid, name))
            blocks.append(np.frombuffer(blk, np.uint8))
        for k, blk in enumerate(random_blocks(rng, mid, N_RANDOM)):
            names.append("mode %#04x random %d" % (mid, k))
            blocks.append(blk)
    for id5 in range(32):                     # every five-bit id, the reserved ones included
        for k in range(8):
            blk = rng.integers(0, 256, 16, dtype=np.uint8)
            blk[0] = (blk[0] & 0xE0) | id5
            names.append("id %#04x random %d" % (id5, k))
            blocks.append(blk)
    for id5 in RESERVED:                      # and a reserved id over all ones
        names.append("id %#04x ones" % id5)
        blocks.append(np.frombuffer(bytes([0xE0 | id5] + [0xFF] * 15), np.uint8))
    out = np.stack(blocks)
    out.setflags(write=False)
    return tuple(names), out


@functools.lru_cache(maxsize=None)
def expected(signed):
    """The model's answer for every case: uint16 [n, 16, 3], computed once and shared."""
    out = decode_blocks(all_cases()[1], signed)
    out.setflags(write=False)
    return out


def mode_of(block):
    b0 = int(block[0])
    return b0 & 3 if (b0 & 3) < 2 else b0 & 31
