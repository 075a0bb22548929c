"""The lookup columns on the device (gl_sort_canonical / gl_lookup_permuted_cols / gl_stark_fill_lookups, csrc/lookup.hip) against
tests/lookup_ref.py, bit for bit, and the STARK "L" of tests/lookup_instances.py from a trace whose lookup columns the device
fills to a proof that equals tests/stark_ref.py's of the host-filled trace. The lengths follow the constants of csrc/lookup.h."""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_instances as ci  # noqa: E402
import ctl_ref as cr  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import lookup_instances as li  # noqa: E402
import lookup_ref as lr  # noqa: E402
import representatives as rp  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401
from plonky2_gpu_amd import stark as ps  # noqa: E402
from test_lookup_ref import HAND_WORKED  # noqa: E402

P = lr.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASHERS = {"poseidon": gr.PoseidonHasher(), "keccak": gr.KeccakHasher()}


def _constant(name):
    text = open(os.path.join(ROOT, "plonky2_gpu_amd", "csrc", "lookup.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


SORT_TILE, SCAN_BLOCK = _constant("LOOKUP_SORT_TILE"), _constant("LOOKUP_SCAN_BLOCK")
# one key more than a sort tile; more than two scan blocks of the n + 1 flags (and four of the 2 n events), a multiple of neither
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, SORT_TILE + 1, 2 * SCAN_BLOCK + 3, (1 << 16) + 3, 1 << 20]
assert (2 * SCAN_BLOCK + 3) % SORT_TILE and (2 * SCAN_BLOCK + 3) % SCAN_BLOCK


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _words(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


def _range_check(rng, n):
    return rng.integers(0, n, size=n, dtype=np.uint64), np.arange(n, dtype=np.uint64)


def _all_equal(rng, n):  # one value in both of its representations
    return np.full(n, 3 + P, dtype=np.uint64), np.full(n, 3, dtype=np.uint64)


def _permutation(rng, n):
    table = _words(rng, n)
    return table[rng.permutation(n)], table


def _below(rng, n):
    return rng.integers(0, 1000, size=n, dtype=np.uint64), (1 << 40) + rng.integers(0, n, size=n, dtype=np.uint64)


def _above(rng, n):
    table, inputs = _below(rng, n)
    return inputs, table


def _long_runs(rng, n):
    values = np.array([7, 1 << 33, 5, P - 1, 1 << 20], dtype=np.uint64)
    return values[rng.integers(0, 4, size=n)], values[rng.integers(1, 5, size=n)]


def _representatives(rng, n):
    """full-width words, the edges of the field, and for everything small enough its second representative x + p"""
    special = np.array([P, P + 1, (1 << 64) - 1, 0, 1, P - 1] + [rp.lift_scalar(x) for x in rp.EDGES], dtype=np.uint64)

    def column():
        col, _ = rp.lift(rp.field_data(rng, n), rng)
        where = rng.random(n) < 0.2
        col[where] = special[rng.integers(0, len(special), size=n)][where]
        return np.where(rng.random(n) < 0.3, _words(rng, n), col).astype(np.uint64)

    table = column()
    return np.where(rng.random(n) < 0.6, table[rng.integers(0, n, size=n)], column()).astype(np.uint64), table


def _top_byte(rng, n):  # only the last radix pass has anything to do
    f = lambda: (rng.integers(0, 255, size=n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00ABCDEF01234567)  # noqa: E731
    return f(), f()


def _low_byte(rng, n):  # only the first
    f = lambda: rng.integers(0, 256, size=n, dtype=np.uint64) | np.uint64(0x1234567890ABCD00)  # noqa: E731
    return f(), f()


FAMILIES = {"range_check": _range_check, "all_equal": _all_equal, "permutation": _permutation, "below": _below, "above": _above,
            "long_runs": _long_runs, "representatives": _representatives, "top_byte": _top_byte, "low_byte": _low_byte}


@functools.lru_cache(maxsize=4)
def _case(family, n):
    """(inputs, table, permuted_inputs, permuted_table): the reference is computed once and never changed"""
    rng = np.random.default_rng(sorted(FAMILIES).index(family) * 1000003 + n)
    inputs, table = (_u64(a) for a in FAMILIES[family](rng, n))
    pi, pt = (_u64(a) for a in lr.permuted_cols(inputs.tolist(), table.tolist()))
    for a in (inputs, table, pi, pt):
        a.setflags(write=False)
    return inputs, table, pi, pt


def _device_permuted_cols(gpu, inputs, table, scratch=None):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import lookup

    n = len(inputs)
    d_in, d_t = pg.DeviceBuffer.from_host(gpu, inputs), pg.DeviceBuffer.from_host(gpu, table)
    d_pi, d_pt = lookup.permuted_cols(gpu, d_in, d_t, n, scratch=scratch)
    out = d_pi.download(), d_pt.download()
    assert (d_in.download() == inputs).all() and (d_t.download() == table).all(), "the inputs are left untouched"
    for b in (d_in, d_t, d_pi, d_pt):
        b.free()
    return out


def _first_difference(got, exp):
    bad = np.flatnonzero(got != exp)
    return None if bad.size == 0 else (int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]), int(bad.size))


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_permuted_cols_and_sort_equal_the_reference(gpu, family, n):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import lookup

    inputs, table, exp_pi, exp_pt = _case(family, n)
    pi, pt = _device_permuted_cols(gpu, inputs, table)
    assert _first_difference(pi, exp_pi) is None, ("permuted_inputs: (index, got, expected, how many)", _first_difference(pi, exp_pi))
    assert _first_difference(pt, exp_pt) is None, ("permuted_table: (index, got, expected, how many)", _first_difference(pt, exp_pt))
    d_in, d_out = pg.DeviceBuffer.from_host(gpu, table), pg.DeviceBuffer(gpu, n)
    lookup.sort_canonical(gpu, d_in, n, out=d_out)
    got = d_out.download()
    exp = _u64(lr.sort_canonical(table.tolist()))
    assert _first_difference(got, exp) is None, ("gl_sort_canonical: (index, got, expected, how many)", _first_difference(got, exp))
    assert (d_in.download() == table).all()
    d_in.free(), d_out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("inputs,table,expected", HAND_WORKED)
def test_the_hand_worked_cases(gpu, inputs, table, expected):
    pi, pt = _device_permuted_cols(gpu, _u64(inputs), _u64(table))
    assert pi.tolist() == sorted(inputs) and pt.tolist() == expected


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1000, SORT_TILE + 1, (1 << 16) + 3])
def test_sort_in_place_and_of_sorted_and_reverse_sorted_keys(gpu, n):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import lookup

    rng = np.random.default_rng(n)
    words = _representatives(rng, n)[0]
    exp = _u64(lr.sort_canonical(words.tolist()))
    scratch = pg.DeviceBuffer(gpu, lookup.scratch_words(n))
    for name, keys in (("random", words), ("sorted", exp), ("reverse sorted", exp[::-1]), ("sorted, lifted", rp.lift(exp, rng)[0])):
        d = pg.DeviceBuffer.from_host(gpu, keys)
        assert lookup.sort_canonical(gpu, d, n, scratch=scratch) is d  # d_out == d_in
        assert _first_difference(d.download(), exp) is None, (name, _first_difference(d.download(), exp))
        d.free()
    scratch.free()


@pytest.mark.gpu
def test_fill_lookups_writes_the_permuted_columns_and_nothing_else(gpu):
    """two lookups that share their table column, n no power of two, a padded pitch; the whole buffer is compared"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import lookup

    n, stride, num_columns = 1000, 1000 + 7, 8
    rng = np.random.default_rng(77)
    host = _words(rng, num_columns * stride).reshape(num_columns, stride)  # the padding and the unused columns hold random words
    host[0, :n] = np.arange(n)
    host[1, :n] = rng.integers(0, n, size=n)
    host[5, :n] = rng.integers(0, n + 20, size=n)  # some inputs the table does not hold
    lookups = [(1, 0, 2, 3), (5, 0, 7, 4)]
    exp = host.copy()
    for c_in, c_t, c_pi, c_pt in lookups:
        exp[c_pi, :n], exp[c_pt, :n] = lr.permuted_cols(host[c_in, :n].tolist(), host[c_t, :n].tolist())
    d = pg.DeviceBuffer.from_host(gpu, host)
    lookup.fill_lookups(gpu, d, n, num_columns, lookups, trace_stride=stride)
    got = d.download().reshape(num_columns, stride)
    assert (got == exp).all(), np.argwhere(got != exp)[:5].tolist()
    d.free()


@pytest.mark.gpu
def test_a_scratch_buffer_holds_nothing_between_calls(gpu):
    """two calls with different inputs on one scratch buffer, then the first again on a scratch buffer of 0xFF bytes and on a zeroed
    one: every call gives its own result"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import lookup

    n = 2 * SCAN_BLOCK + 3
    words = lookup.scratch_words(n)
    scratch = pg.DeviceBuffer(gpu, words)
    for family in ("representatives", "range_check", "representatives"):
        inputs, table, exp_pi, exp_pt = _case(family, n)
        pi, pt = _device_permuted_cols(gpu, inputs, table, scratch=scratch)
        assert (pi == exp_pi).all() and (pt == exp_pt).all(), family
    inputs, table, exp_pi, exp_pt = _case("long_runs", n)
    for fill in (0xFF, 0x00):
        scratch.upload(np.full(words, fill * 0x0101010101010101, dtype=np.uint64))
        pi, pt = _device_permuted_cols(gpu, inputs, table, scratch=scratch)
        assert (pi == exp_pi).all() and (pt == exp_pt).all(), hex(fill)
    scratch.free()


def test_the_scratch_size_is_what_the_header_promises():
    """no device needed: at most 12 n words, and for large n the 8.7 n of the header's comment"""
    from plonky2_gpu_amd import lookup

    for n in (1, 1000, 1 << 20, 1 << 30):
        assert lookup.scratch_words(n) <= 12 * n + 4096
    assert lookup.scratch_words(1 << 20) <= 9 * (1 << 20)
    for n in (0, (1 << 30) + 1):
        with pytest.raises(ValueError):
            lookup.scratch_words(n)


@pytest.mark.gpu
def test_refusals(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    n = 100
    a, b, c, d = (pg.DeviceBuffer(gpu, 2 * n) for _ in range(4))
    scratch = pg.DeviceBuffer(gpu, _lib.load().gl_lookup_scratch_bytes(n) // 8)

    def refused(message, name, *args):
        with pytest.raises(pg.Plonky2HipError, match=re.escape(message)) as e:
            _lib.call(name, *args)
        assert e.value.code == pg.GL_E_INVALID and name in str(e.value)

    assert _lib.load().gl_lookup_scratch_bytes(0) == 0 and _lib.load().gl_lookup_scratch_bytes((1 << 30) + 1) == 0
    for bad_n in (0, (1 << 30) + 1):
        refused("n must be in 1 ..= 2^30", "gl_sort_canonical", a.ptr, b.ptr, bad_n, scratch.ptr, gpu.ptr)
        refused("n must be in 1 ..= 2^30", "gl_lookup_permuted_cols", a.ptr, b.ptr, bad_n, c.ptr, d.ptr, scratch.ptr, gpu.ptr)
        refused("n must be in 1 ..= 2^30", "gl_stark_fill_lookups", a.ptr, n, bad_n, 1, None, 0, scratch.ptr, gpu.ptr)
    for args in ((None, b.ptr, n, scratch.ptr, gpu.ptr), (a.ptr, None, n, scratch.ptr, gpu.ptr), (a.ptr, b.ptr, n, None, gpu.ptr),
                 (a.ptr, b.ptr, n, scratch.ptr, None)):
        refused("null pointer", "gl_sort_canonical", *args)
    good = [a.ptr, b.ptr, n, c.ptr, d.ptr, scratch.ptr, gpu.ptr]
    for k in (0, 1, 3, 4, 5, 6):
        refused("null pointer", "gl_lookup_permuted_cols", *[None if i == k else x for i, x in enumerate(good)])
    lookups = np.array([1, 0, 2, 3], dtype=np.uint32)
    refused("null pointer", "gl_stark_fill_lookups", None, n, n, 4, lookups, 1, scratch.ptr, gpu.ptr)
    refused("null pointer", "gl_stark_fill_lookups", a.ptr, n, n, 4, None, 1, scratch.ptr, gpu.ptr)
    refused("null pointer", "gl_stark_fill_lookups", a.ptr, n, n, 4, lookups, 1, None, gpu.ptr)
    refused("null pointer", "gl_stark_fill_lookups", a.ptr, n, n, 4, lookups, 1, scratch.ptr, None)
    refused("d_scratch must be 16-byte aligned", "gl_sort_canonical", a.ptr, b.ptr, n, scratch.ptr + 8, gpu.ptr)
    # overlaps: the n-word ranges
    refused("d_out overlaps d_in without being d_in", "gl_sort_canonical", a.ptr, a.at(n - 1), n, scratch.ptr, gpu.ptr)
    refused("d_out overlaps d_in without being d_in", "gl_sort_canonical", a.at(1), a.ptr, n, scratch.ptr, gpu.ptr)
    _lib.call("gl_sort_canonical", a.ptr, a.at(n), n, scratch.ptr, gpu.ptr)  # adjacent ranges do not overlap
    refused("the two outputs overlap", "gl_lookup_permuted_cols", a.ptr, b.ptr, n, c.ptr, c.at(n - 1), scratch.ptr, gpu.ptr)
    refused("the two outputs overlap", "gl_lookup_permuted_cols", a.ptr, b.ptr, n, c.ptr, c.ptr, scratch.ptr, gpu.ptr)
    refused("an output overlaps an input", "gl_lookup_permuted_cols", a.ptr, b.ptr, n, a.ptr, d.ptr, scratch.ptr, gpu.ptr)
    refused("an output overlaps an input", "gl_lookup_permuted_cols", a.ptr, b.ptr, n, c.ptr, b.at(n - 1), scratch.ptr, gpu.ptr)
    refused("an output overlaps an input", "gl_lookup_permuted_cols", a.ptr, b.ptr, n, a.at(n - 1), d.ptr, scratch.ptr, gpu.ptr)
    _lib.call("gl_lookup_permuted_cols", a.ptr, a.ptr, n, c.ptr, d.ptr, scratch.ptr, gpu.ptr)  # the two inputs may be one column
    # the trace form
    trace = pg.DeviceBuffer(gpu, 4 * n)
    refused("column out of range", "gl_stark_fill_lookups", trace.ptr, n, n, 3, lookups, 1, scratch.ptr, gpu.ptr)
    refused("column out of range", "gl_stark_fill_lookups", trace.ptr, n, n, 4, np.array([4, 0, 2, 3], dtype=np.uint32), 1, scratch.ptr, gpu.ptr)
    refused("trace_stride smaller than n", "gl_stark_fill_lookups", trace.ptr, n - 1, n, 4, lookups, 1, scratch.ptr, gpu.ptr)
    for bad in ([1, 0, 1, 3], [1, 0, 2, 0], [1, 0, 2, 2], [1, 0, 2, 3, 1, 0, 3, 2], [1, 0, 2, 3, 2, 0, 1, 3]):
        flat = np.array(bad, dtype=np.uint32)
        refused("a permuted column is also an input, table or permuted column of the call", "gl_stark_fill_lookups", trace.ptr, n, n, 4, flat,
                len(bad) // 4, scratch.ptr, gpu.ptr)
    gpu.synchronize()
    for buf in (a, b, c, d, scratch, trace):
        buf.free()


# ---------------------------------------------------------------- end to end: fill on the device, prove on the device
_FRI = {4: dict(rate_bits=1, cap_height=1, arity_bits=(2,)), 6: dict(rate_bits=2, cap_height=2, arity_bits=(3,)),
        12: dict(rate_bits=1, cap_height=2, arity_bits=(3, 3))}


@functools.lru_cache(maxsize=None)
def _l_reference(degree_bits, hasher):
    """(the trace with its lookup columns filled on the host, the reference's proof of it, its bytes)"""
    from oracle import accel

    trace, _ = li.L.make_trace(degree_bits, seed=degree_bits)
    with accel.c_backend():
        proof = sr.prove(HASHERS[hasher], li.L, li.NUM_CHALLENGES[hasher], si.fri_params(**_FRI[degree_bits]), trace, [])
    return trace, proof, sr.proof_bytes(HASHERS[hasher], proof)


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits", [4, 6, 12])
@pytest.mark.parametrize("hasher", ["poseidon", "keccak"])
def test_l_filled_and_proved_on_the_device_equals_the_reference(gpu, hasher, degree_bits):
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import lookup
    from plonky2_gpu_amd import stark as pstark

    n, nch, fp = 1 << degree_bits, li.NUM_CHALLENGES[hasher], si.fri_params(**_FRI[degree_bits])
    filled, _, exp = _l_reference(degree_bits, hasher)
    host = _u64(filled)
    host[li.PV] = host[li.PT] = 0
    d_trace = pg.DeviceBuffer.from_host(gpu, host)
    scratch = pg.DeviceBuffer(gpu, lookup.scratch_words(n))
    ns = pg.NativeStark(gpu, li.L.desc(degree_bits, nch, fp), hasher)
    try:
        lookup.fill_lookups(gpu, d_trace, n, li.L.num_columns, li.LOOKUPS, scratch=scratch)  # queued; the proof follows on the same stream
        data = ns.prove_bytes(d_trace, [])
        assert (d_trace.download().reshape(6, n) == _u64(filled)).all()
        assert data == exp
    finally:
        ns.close()
    parsed = pstark.proof_from_bytes(data, ns.desc, hasher)
    with accel.c_backend():
        assert sr.verify(HASHERS[hasher], li.L, nch, fp, parsed)
    d_trace.free(), scratch.free()


def _w_program():
    a = ps.StarkAsm()
    a.emit_transition(a.sub(a.next(1), a.add(a.local(1), a.imm(1))))
    a.emit_transition(a.sub(a.sub(a.next(2), a.local(2)), a.mul(a.local(0), a.local(1))))
    return a


def _w_closure(F, l, n, pis, c):
    c.constraint_transition(F.sub(n[1], F.add(l[1], F.one)))
    c.constraint_transition(F.sub(F.sub(n[2], l[2]), F.mul(l[0], l[1])))


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", ["poseidon", "keccak"])
def test_a_table_with_a_lookup_inside_a_two_table_proof(gpu, hasher):
    """table 0 is L (its counter looks into table 1 without a filter), table 1 holds the counter's values in another order in
    column 0 beside two constrained columns and two free ones"""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import lookup

    degree_bits, nch = 4, li.NUM_CHALLENGES[hasher]
    n = 1 << degree_bits
    tables = [ci.Table("L", 6, 3, li.L.pairs, li.l_program(), li.l_closure), ci.Table("W", 5, 3, [], _w_program(), _w_closure)]
    lookups = [ps.CrossTableLookup([ps.TableWithColumns(0, [ps.CtlColumn.single(li.C0)])], ps.TableWithColumns(1, [ps.CtlColumn.single(0)]))]
    system = ci.System(tables, lookups, None)
    fp = ci.fri_params(rate_bits=1, cap_height=1, arity_bits=((2,), (2,)))
    rng = np.random.default_rng(31)
    filled = li.L.make_trace(degree_bits, seed=3)[0]
    w0, w1, w2 = [int(x) for x in rng.permutation(n)], [9 + r for r in range(n)], [4]
    for r in range(n - 1):
        w2.append((w2[r] + w0[r] * w1[r]) % P)
    w = [w0, w1, w2, [int(x) for x in _words(rng, n) % np.uint64(P)], [int(x) for x in _words(rng, n) % np.uint64(P)]]
    with accel.c_backend():
        exp = cr.proofs_bytes(HASHERS[hasher], cr.prove_tables(HASHERS[hasher], system, nch, fp, [filled, w]))
    host = _u64(filled)
    host[li.PV] = host[li.PT] = 0
    d_trace, scratch = pg.DeviceBuffer.from_host(gpu, host), pg.DeviceBuffer(gpu, lookup.scratch_words(n))
    desc = system.desc((degree_bits, degree_bits), nch, fp)
    nt = pg.NativeStarkTables(gpu, desc, hasher)
    try:
        lookup.fill_lookups(gpu, d_trace, n, 6, li.LOOKUPS, scratch=scratch)
        data = nt.prove_bytes([d_trace, _u64(w)])
        assert data == exp
    finally:
        nt.close()
    with accel.c_backend():
        assert cr.verify_tables(HASHERS[hasher], system, nch, fp, ps.tables_proof_from_bytes(data, desc, hasher))
    d_trace.free(), scratch.free()
