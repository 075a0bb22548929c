"""The four-instruction subtraction (gl_field.h sub_f / bfly_f: d = a - b with borrow B, then dh - B and dl + B separately) against
Python big integers: operands that make the carry of dl + B into the high word go missing (low word of a - b = 2^32 - 1 under a
borrow), operands with a true second borrow (high word of a - b = 0 under a borrow), both at once — alone, in every position of a
group of three, and at every butterfly of every stage of the register-level radix routines, where the pending correction goes
through the stage's shift as the constant 2^(32 + K) or e 2^K."""
import numpy as np
import pytest

from gpu_util import P, gpu  # noqa: F401

M64 = (1 << 64) - 1


def run_op(gpu, op, a, b=None):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    da = pg.DeviceBuffer.from_host(gpu, a)
    db = pg.DeviceBuffer.from_host(gpu, b) if b is not None else None
    do = pg.DeviceBuffer(gpu, len(a))
    _lib.call("gl_debug_field_op", op, da.ptr, db.ptr if db else None, do.ptr, len(a), gpu.ptr)
    return do.download().tolist()


def flagged_pairs():
    """(a, b, kind) with a < b, d = a - b + 2^64: kind "carry" (low word of d all ones, high word not 0), "borrow" (high word 0, low
    word not all ones), "both" (d = 2^32 - 1)."""
    out = []
    targets = [((h << 32) | 0xFFFFFFFF, "carry") for h in (1, 0x12345678, 0xFFFFFFFE, 0xFFFFFFFF)]
    targets += [(low, "borrow") for low in (1, 2, 0x80000000, 0xFFFFFFFE)]
    targets += [(0xFFFFFFFF, "both")]
    rng = np.random.default_rng(41)
    for d, kind in targets:
        gap = (1 << 64) - d                       # b - a
        bs = [M64, gap, P if P >= gap else M64, P + 1 if P + 1 >= gap else M64 - 1]
        bs += [int(x) for x in rng.integers(gap, 1 << 64, size=3, dtype=np.uint64, endpoint=False)] if gap < (1 << 64) - 1 else []
        for b in bs:
            if gap <= b <= M64:
                out.append((b - gap, b, kind))
    out += [(0, M64, "borrow"), (P + 5, P + 6, "carry"), (P, P + 1, "carry")]   # a = 0 and b = 2^64 - 1; both operands >= p
    for a, b, kind in out:
        d = (a - b) % (1 << 64)
        assert a < b and {"carry": (d & 0xFFFFFFFF) == 0xFFFFFFFF and d >> 32 != 0, "borrow": d >> 32 == 0 and (d & 0xFFFFFFFF) != 0xFFFFFFFF,
                          "both": d == 0xFFFFFFFF}[kind], (a, b, kind)
    return out


def test_the_flagged_pairs_cover_the_three_cases():
    kinds = {k for _, _, k in flagged_pairs()}
    assert kinds == {"carry", "borrow", "both"}


@pytest.mark.gpu
def test_subtraction_alone_and_in_every_position_of_its_group(gpu):
    """op 1 (gl::sub, unchanged) and ops 21-23 (sub_f + sub_fix in a group of three: (x, y), (y, x), (x ^ y, x), the member `which`
    returned). Every flagged pair is given as member 0, 1 and 2 of its group, so that the correction runs beside unflagged
    neighbours first, in the middle and last; and 2^16 random pairs."""
    pairs = [(a, b) for a, b, _ in flagged_pairs()]
    rng = np.random.default_rng(42)
    rnd = [(int(x), int(y)) for x, y in rng.integers(0, 1 << 64, size=(1 << 16, 2), dtype=np.uint64, endpoint=False).tolist()]
    # (x, y) such that member m of the group computes a - b
    arrange = [lambda a, b: (a, b), lambda a, b: (b, a), lambda a, b: (b, a ^ b)]
    members = [lambda x, y: (x, y), lambda x, y: (y, x), lambda x, y: (x ^ y, x)]
    xy = [arr(a, b) for arr in arrange for a, b in pairs] + rnd
    for m, arr in enumerate(arrange):
        for a, b in pairs[:4]:
            assert members[m](*arr(a, b)) == (a, b)
    x = np.array([p[0] for p in xy], dtype=np.uint64)
    y = np.array([p[1] for p in xy], dtype=np.uint64)
    assert run_op(gpu, 1, x, y) == [(a - b) % P for a, b in xy]
    for which, m in enumerate(members):
        exp = [(m(a, b)[0] - m(a, b)[1]) % P for a, b in xy]
        assert run_op(gpu, 21 + which, x, y) == exp, which


def _dif_stage(v, s, d=4):
    """One radix-2 stage of the in-register DIF butterflies (ntt_kernels.h radix_dif_stage): blocks of 2^d slots, stage s."""
    half = 1 << s
    out = list(v)
    for base in range(0, 16, 1 << d):
        for bb in range((1 << d) // 2):
            i0 = base + (bb // half) * 2 * half + (bb % half)
            i1 = i0 + half
            k = (39 * (bb % half) * (32 >> s)) % 192
            a, c = v[i0], v[i1]
            out[i0] = (a + c) % P
            out[i1] = (a - c) * pow(2, k, P) % P
    return out


def _dif16(r):
    for s in (3, 2, 1, 0):
        r = _dif_stage(r, s)
    return r


def _dif4_blocks(r):
    return _dif_stage(_dif_stage(r, 1, d=2), 0, d=2)


@pytest.fixture(scope="module")
def stage_vectors():
    """Vectors of sixteen. For every stage s, every butterfly (i0, i0 + 2^s) of that stage and every flagged pair: the pair in the
    butterfly's two slots, in both orders (a twiddle 2^K with K >= 96 swaps the operands of the subtraction), the other slots random;
    the same with the slots above i0 + 2^s zero, which carries the pair unchanged (x + 0 and x - 0 keep their bits, slot 0's
    twiddle is 1) through the earlier stages of radix_dif to stage s; and vectors whose every butterfly of a stage is flagged."""
    pairs = [(a, b) for a, b, _ in flagged_pairs()]
    rng = np.random.default_rng(43)
    vecs = []
    for s in range(4):
        half = 1 << s
        for bb in range(8):
            i0 = (bb // half) * 2 * half + (bb % half)
            for a, b in pairs:
                for lo, hi in ((a, b), (b, a)):
                    v = [int(x) for x in rng.integers(0, 1 << 64, size=16, dtype=np.uint64, endpoint=False)]
                    v[i0], v[i0 + half] = lo, hi
                    vecs.append(v)
        for a, b in pairs:      # reaches stage s of radix_dif / radix_dif_blocks / the radix 4 with its bits intact
            for lo, hi in ((a, b), (b, a)):
                v = [0] * 16
                v[0], v[half] = lo, hi
                vecs.append(v)
            v = [0] * 16        # every butterfly of the stage, neighbours flagged too
            for bb in range(8):
                i0 = (bb // half) * 2 * half + (bb % half)
                v[i0], v[i0 + half] = (a, b) if bb % 2 == 0 else (b, a)
            vecs.append(v)
    while len(vecs) % 64:
        vecs.append([0] * 16)
    return vecs


@pytest.mark.gpu
def test_radix_routines_settle_the_pending_correction_through_every_shift(gpu, stage_vectors):
    """ops 100-109: radix_dif_stage<4, 0, s>, radix_dif<4, 0>, radix_dif_blocks<2>, shift_twiddles_radix4<k>. The pending correction
    of a difference (+ 2^32 or - e) goes through the stage's shift 2^K: every K the stages use (stage s, butterfly j: 39 j (32 >> s)
    mod 96) is met by a flagged butterfly in the vectors above."""
    rows = stage_vectors
    flat = np.array(rows, dtype=np.uint64).reshape(-1)

    def run(which):
        return np.array(run_op(gpu, 100 + which, flat), dtype=np.uint64).reshape(len(rows), 16).tolist()

    for s in range(4):
        assert run(s) == [_dif_stage(r, s) for r in rows], ("stage", s)
    assert run(4) == [_dif16(r) for r in rows]
    assert run(5) == [_dif4_blocks(r) for r in rows]
    for kbhi in range(4):
        exp = [_dif4_blocks([x * pow(2, 39 * (i & 3) * (4 * kbhi + (i >> 2)), P) % P for i, x in enumerate(r)]) for r in rows]
        assert run(6 + kbhi) == exp, ("shift twiddles + radix 4", kbhi)
