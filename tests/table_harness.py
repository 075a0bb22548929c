"""What the four tests/test_gpu_*_table.py files share: the proving checks of one table proved alone by gl_stark_prove from its
device-built trace, against tests/stark_ref.py byte for byte. A test file describes its table in a Table record and its test
functions call in here; what only one table checks stays in its file."""
import threading

import numpy as np
import pytest

import generic_prove_ref as gr
import stark_instances as si
import stark_ref as sr
from strided import Strided

HASHERS = {"poseidon": gr.PoseidonHasher(), "keccak": gr.KeccakHasher()}
FP = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,))
REJECTED_AT_ZETA = "Mismatch between evaluation and opening"


def first_difference(got, exp):
    bad = np.argwhere(got != exp)
    return None if bad.size == 0 else ("first (column, row) that differs", bad[0].tolist(), len(bad), hex(int(got[tuple(bad[0])])), hex(int(exp[tuple(bad[0])])))


class System:
    """tests/ctl_ref.py's view of a system of tables"""

    def __init__(self, tables, lookups):
        self.tables, self.lookups, self.ctl_closures = tables, lookups, None


class Table:
    """module: the table's module in plonky2_gpu_amd, by name (imported when first used); stark_class: the reference's STARK of
    tests/<table>_ref.py, built from the module's program(); reference_trace(n): the provable trace of n rows as [columns][n],
    never changed; device_trace(ctx, n): the same trace built on the device; sizes: the n that are provable; flip(module) ->
    (column, row): the cell of the smallest trace whose flipped low bit the verifier refuses with flip_message."""

    def __init__(self, module, stark_class, columns, sizes, reference_trace, device_trace, flip, flip_message=REJECTED_AT_ZETA):
        self.module_name, self.stark_class, self.columns, self.sizes = module, stark_class, columns, sizes
        self.reference_trace, self.device_trace, self.flip, self.flip_message = reference_trace, device_trace, flip, flip_message
        self._stark, self._proofs = None, {}

    @property
    def module(self):
        import importlib

        return importlib.import_module("plonky2_gpu_amd." + self.module_name)

    def stark(self):
        if self._stark is None:
            instrs, immediates = self.module.program()
            self._stark = self.stark_class(instrs, immediates)
        return self._stark

    def desc(self, n, num_challenges):
        return self.module.stark_desc(n.bit_length() - 1, num_challenges, FP)

    def reference_proof(self, hasher, num_challenges, n):
        """tests/stark_ref.py's proof of reference_trace(n), computed once"""
        from oracle import accel

        key = (hasher, num_challenges, n)
        if key not in self._proofs:
            trace = [[int(v) for v in col] for col in self.reference_trace(n)]
            with accel.c_backend():
                self._proofs[key] = sr.proof_bytes(HASHERS[hasher], sr.prove(HASHERS[hasher], self.stark(), num_challenges, FP, trace, []))
        return self._proofs[key]


def check_proof_bytes(t, gpu, hasher, num_challenges, n, compiled=False, verify=None):
    """the device's proof of the device-built trace is the reference's, again on recycled buffers, and parses back to its bytes;
    `verify`: the evaluator with which tests/stark_ref.py's verifier must accept it as well"""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    exp = t.reference_proof(hasher, num_challenges, n)
    ns = pg.NativeStark(gpu, t.desc(n, num_challenges), hasher, compiled=compiled, unit_instrs=0 if compiled else None)
    try:
        assert bool(ns.is_compiled) == compiled
        d_trace = t.device_trace(gpu, n)
        data = ns.prove_bytes(d_trace, [])
        assert data == exp
        assert ns.prove_bytes(d_trace, []) == exp  # on recycled buffers
    finally:
        ns.close()
    parsed = pstark.proof_from_bytes(data, ns.desc, hasher)
    assert pstark.proof_to_bytes(parsed, ns.desc, hasher) == data
    if verify:
        with accel.c_backend():
            assert sr.verify(HASHERS[hasher], t.stark(), num_challenges, FP, parsed, evaluator=verify)


def check_quotient_polys(t, gpu, lde, alphas, zs=None, sets=None):
    """gl_stark_quotient_polys on the words `lde` [columns][64] in place of the LDEs of a 32-row trace (and `zs`, `sets` in place
    of the permutation Zs and their challenges) against tests/stark_ref.py on the same words reduced, at the tight and at a padded
    column pitch; every constraint non-zero; the inputs are left as they were"""
    import plonky2_gpu_amd as pg

    P = 0xFFFFFFFF00000001
    leaves = lambda a: [[int(v) % P for v in row] for row in a.T]  # noqa: E731
    exp = np.array(sr.compute_quotient_polys(t.stark(), 2, 5, 1, leaves(lde), None if zs is None else leaves(zs), sets, [], alphas), dtype=np.uint64)
    assert exp.shape == (2, 64) and exp.all()
    ns = pg.NativeStark(gpu, t.desc(32, 2))
    try:
        for stride in (64, 64 + 6):
            bufs = [Strided(gpu, a, stride) for a in ([lde] if zs is None else [lde, zs])]
            got = ns.quotient_polys(bufs[0].ptr, None if zs is None else bufs[1].ptr, stride, alphas, sets, [])
            assert all((b.polys() == a).all() for b, a in zip(bufs, (lde, zs)))
            for b in bufs:
                b.free()
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("column pitch", stride, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad))
    finally:
        ns.close()


def check_flipped_cell_is_rejected(t, gpu, verifier):
    """The device proves the trace with the low bit of t.flip's cell flipped, as the reference's prover does (quotient_degree_factor
    2 is a power of two: its trim cannot fail), and the verifier refuses the proof with t.flip_message. `verifier`: "stark_ref":
    tests/stark_ref.py's on the parsed proof; "stark_verify": tests/stark_verify.py's on the bytes, which must first accept the
    proof of the untouched trace."""
    import plonky2_gpu_amd as pg
    import stark_verify
    from plonky2_gpu_amd import stark as pstark

    n = min(t.sizes)
    ns = pg.NativeStark(gpu, t.desc(n, 2))
    try:
        d_trace = t.device_trace(gpu, n)
        if verifier == "stark_verify":
            assert stark_verify.accepts(ns.desc, ns.prove_bytes(d_trace, []))
        column, row = t.flip(t.module)
        cell = d_trace.download(column * n + row, 1)
        assert cell[0] == t.reference_trace(n)[column, row]
        d_trace.upload(cell ^ np.uint64(1), column * n + row)
        data = ns.prove_bytes(d_trace, [])
        parsed = pstark.proof_from_bytes(data, ns.desc)
    finally:
        ns.close()
    with pytest.raises(AssertionError, match=t.flip_message):
        if verifier == "stark_verify":
            stark_verify.accepts(ns.desc, data)
        else:
            sr.verify(HASHERS["poseidon"], t.stark(), 2, FP, parsed)


def check_two_contexts_on_two_threads(t, gpu):
    """one handle, two contexts, two threads: each builds the smallest trace and proves it twice; every proof is the reference's"""
    import plonky2_gpu_amd as pg

    n = min(t.sizes)
    exp = t.reference_proof("poseidon", 2, n)
    ns = pg.NativeStark(gpu, t.desc(n, 2))
    other = pg.Context(0)
    try:
        alone = ns.prove_bytes(t.device_trace(gpu, n), [])
        assert alone == exp
        got, errors = [None, None], []

        def work(k, ctx):
            try:
                for _ in range(2):
                    got[k] = ns.prove_bytes(t.device_trace(ctx, n), [], ctx=ctx)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(k, ctx)) for k, ctx in enumerate((gpu, other))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert got == [alone, alone]
    finally:
        ns.close()
        other.close()
