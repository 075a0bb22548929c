"""STARKs: starky's prove() on the device (gl_stark_create / gl_stark_prove, csrc/prove.hip and csrc/stark.hip).

A STARK is described by its shape, its permutation pairs and ONE register program for all its constraints — what a host derives from
`Stark::eval_packed_generic` (starky/src/stark.rs) the way the gate programs are derived from `eval_unfiltered_*`. The program uses
the instruction set of gate_program.py with the STARK opcodes of include/plonky2_hip.h:

    LOAD_WIRE  dst <- local_values[a]          LOAD_NEXT dst <- next_values[a]          LOAD_PI dst <- public_inputs[a]
    EMIT            yield_constr.constraint(r[a])
    EMIT_TRANSITION yield_constr.constraint_transition(r[a])
    EMIT_FIRST_ROW  yield_constr.constraint_first_row(r[a])
    EMIT_LAST_ROW   yield_constr.constraint_last_row(r[a])

LOAD_CONST does not exist in a STARK program. The proof's wire format is defined in the header (the reference has no serializer for
StarkProofWithPublicInputs); proof_to_bytes / proof_from_bytes mirror it."""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceBuffer
from .gate_program import ACC, ACCR, ADD, EMIT, LOAD_CONST, LOAD_IMM, LOAD_PI, LOAD_WIRE, MUL, MULK, SUB, GateAsm, ImmediatePool  # noqa: F401
from .serialization import Buffer

LOAD_NEXT, EMIT_TRANSITION, EMIT_FIRST_ROW, EMIT_LAST_ROW = 11, 12, 13, 14
EMITS = (EMIT, EMIT_TRANSITION, EMIT_FIRST_ROW, EMIT_LAST_ROW)
P = 0xFFFFFFFF00000001


class StarkAsm(GateAsm):
    """Emits a STARK's constraint program: GateAsm's registers, immediates and ACC accumulators (its overflow contract is enforced
    where acc() is called) with the two rows of a STARK and starky's four kinds of constraint."""

    def __init__(self):
        super().__init__(ImmediatePool())

    def local(self, i):
        return self.op(LOAD_WIRE, i)

    def next(self, i):
        return self.op(LOAD_NEXT, i)

    def const(self, i):
        raise ValueError("a STARK has no constants columns: LOAD_CONST is invalid in a STARK program")

    def emit_transition(self, a):
        self.instrs.append((EMIT_TRANSITION, 0, a, 0))

    def emit_first_row(self, a):
        self.instrs.append((EMIT_FIRST_ROW, 0, a, 0))

    def emit_last_row(self, a):
        self.instrs.append((EMIT_LAST_ROW, 0, a, 0))

    def program(self):
        """(instrs [k][4] uint16, immediates list)"""
        return np.array(self.instrs, dtype=np.uint16).reshape(-1, 4), list(self.pool.values)


class StarkDesc:
    """The description of a STARK: `instrs` [k][4] (op, dst, a, b), `immediates`, `pairs` a list of PermutationPair::column_pairs
    (lists of (lhs, rhs) columns), `fri_params` as everywhere in this package (hiding must be false)."""

    def __init__(self, degree_bits, num_columns, num_public_inputs, constraint_degree, num_challenges, fri_params, instrs, immediates=(), pairs=()):
        self.degree_bits, self.num_columns, self.num_public_inputs = degree_bits, num_columns, num_public_inputs
        self.constraint_degree, self.num_challenges, self.fri_params = constraint_degree, num_challenges, dict(fri_params)
        self.instrs = np.ascontiguousarray(np.array(instrs, dtype=np.uint16).reshape(-1, 4))
        self.immediates = [int(x) % P for x in immediates]
        self.pairs = [[(int(a), int(b)) for a, b in pair] for pair in pairs]

    @property
    def quotient_degree_factor(self):  # stark.rs:79-81
        return max(1, self.constraint_degree - 1)

    @property
    def quotient_degree_bits(self):
        return (self.quotient_degree_factor - 1).bit_length()

    @property
    def num_zs(self):  # num_permutation_batches
        return -(-len(self.pairs) * self.num_challenges // self.quotient_degree_factor)

    @property
    def num_quotient_polys(self):
        return self.quotient_degree_factor * self.num_challenges


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


class NativeStark:
    """gl_stark_create: the handle of one STARK on one device; prove_bytes() = gl_stark_prove."""

    def __init__(self, ctx, desc, hasher=_lib.GL_HASHER_POSEIDON):
        self.ctx, self.desc, self.hasher = ctx, desc, _lib.hasher_id(hasher)
        self.ptr = None
        fp = desc.fri_params
        arity = np.ascontiguousarray(fp["reduction_arity_bits"], dtype=np.uint32)
        imms = _u64(desc.immediates) if desc.immediates else None
        flat = np.ascontiguousarray([c for pair in desc.pairs for cp in pair for c in cp], dtype=np.uint32)
        bounds = np.ascontiguousarray(np.cumsum([0] + [len(pair) for pair in desc.pairs]), dtype=np.uint32)
        d = _lib.GlStarkDesc(
            ctypes.sizeof(_lib.GlStarkDesc), desc.degree_bits, desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.num_challenges,
            _lib.GlFriParams(fp["rate_bits"], fp["cap_height"], fp["proof_of_work_bits"], fp["num_query_rounds"], arity.size, arity.ctypes.data,
                             1 if fp.get("hiding") else 0),
            desc.instrs.ctypes.data, desc.instrs.shape[0], imms.ctypes.data if imms is not None else None, 0 if imms is None else imms.size,
            flat.ctypes.data if desc.pairs else None, bounds.ctypes.data if desc.pairs else None, len(desc.pairs))
        h = ctypes.c_void_p()
        _lib.call("gl_stark_create", self.hasher, ctypes.byref(d), ctypes.byref(h), ctx.ptr)
        self.ptr = h.value

    def prove_bytes(self, trace, public_inputs, timing=None, ctx=None):
        """`trace`: host [num_columns][n] value columns or a DeviceBuffer; `ctx`: another context of the handle's device (several host
        threads, each with its own context, may prove with one handle at the same time)."""
        ctx = ctx or self.ctx
        d_t = trace if isinstance(trace, DeviceBuffer) else DeviceBuffer.from_host(ctx, _u64(trace))
        pis = _u64(public_inputs)
        if pis.size != self.desc.num_public_inputs:
            raise ValueError("the STARK has %d public inputs" % self.desc.num_public_inputs)
        out, ln = ctypes.c_void_p(), ctypes.c_uint64()
        ms = np.zeros(_lib.GL_STARK_STAGES, dtype=np.float64) if timing is not None else None
        _lib.call("gl_stark_prove", self.ptr, d_t.ptr, pis, ctypes.byref(out), ctypes.byref(ln), ms, ctx.ptr)
        data = ctypes.string_at(out.value, ln.value)
        _lib.load().gl_bytes_free(out.value)
        if timing is not None:
            for name, v in zip(_lib.STARK_STAGE_NAMES, ms):
                timing[name] = timing.get(name, 0.0) + float(v)
        return data

    def prove(self, trace, public_inputs, timing=None):
        return proof_from_bytes(self.prove_bytes(trace, public_inputs, timing), self.desc, self.hasher)

    def permutation_zs(self, trace, challenge_sets, trace_stride=None):
        """gl_stark_permutation_zs. `trace`: host [num_columns][n] (uploaded at pitch `trace_stride`, default n); `challenge_sets`:
        [qdf][num_challenges] (beta, gamma). Returns [num_zs][n]."""
        n = 1 << self.desc.degree_bits
        stride = trace_stride or n
        host = np.zeros((self.desc.num_columns, stride), dtype=np.uint64)
        host[:, :n] = _u64(trace)
        d_t = DeviceBuffer.from_host(self.ctx, host)
        d_z = DeviceBuffer(self.ctx, self.desc.num_zs * n)
        _lib.call("gl_stark_permutation_zs", self.ptr, d_t.ptr, stride, _challenge_words(challenge_sets), d_z.ptr, self.ctx.ptr)
        return d_z.download().reshape(self.desc.num_zs, n)

    def quotient_polys(self, trace_lde, zs_lde, column_stride, alphas, challenge_sets, public_inputs):
        """gl_stark_quotient_polys. `trace_lde` / `zs_lde`: DeviceBuffers (or pointers into them) holding the column-major LDEs at pitch
        `column_stride`, `zs_lde` None without pairs. Returns the coefficients [num_challenges][n << quotient_degree_bits]."""
        size = 1 << (self.desc.degree_bits + self.desc.quotient_degree_bits)
        d_q = DeviceBuffer(self.ctx, self.desc.num_challenges * size)
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else b)  # noqa: E731
        ch = _challenge_words(challenge_sets) if challenge_sets is not None else None
        _lib.call("gl_stark_quotient_polys", self.ptr, ptr(trace_lde), ptr(zs_lde), column_stride, _u64(alphas), ch, _u64(public_inputs), d_q.ptr,
                  self.ctx.ptr)
        return d_q.download().reshape(self.desc.num_challenges, size)

    def trim(self):
        _lib.call("gl_stark_trim", self.ptr)

    def close(self):
        if self.ptr:
            _lib.load().gl_stark_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _challenge_words(challenge_sets):
    """[set][challenge] (beta, gamma) -> the flat order they are drawn in"""
    return _u64([w for s in challenge_sets for bg in s for w in bg])


def prove(ctx, desc, trace, public_inputs, hasher=_lib.GL_HASHER_POSEIDON):
    """One proof of `trace` (host [num_columns][n] or a DeviceBuffer): the parsed StarkProofWithPublicInputs."""
    s = NativeStark(ctx, desc, hasher)
    try:
        return s.prove(trace, public_inputs)
    finally:
        s.close()


# ---------------------------------------------------------------- wire format (include/plonky2_hip.h, gl_stark_prove)
def proof_to_bytes(proof, desc, hasher=_lib.GL_HASHER_POSEIDON):
    b = Buffer(hasher=hasher)
    b.write_merkle_cap(proof["trace_cap"])
    if desc.pairs:
        b.write_merkle_cap(proof["permutation_zs_cap"])
    b.write_merkle_cap(proof["quotient_polys_cap"])
    op = proof["openings"]
    b.write_field_ext_vec(op["local_values"])
    b.write_field_ext_vec(op["next_values"])
    if desc.pairs:
        b.write_field_ext_vec(op["permutation_zs"])
        b.write_field_ext_vec(op["permutation_zs_next"])
    b.write_field_ext_vec(op["quotient_polys"])
    fp = proof["opening_proof"]  # write_fri_proof
    for cap in fp["commit_phase_merkle_caps"]:
        b.write_merkle_cap(cap)
    for rnd in fp["query_round_proofs"]:
        for evals, siblings in rnd["initial_trees_proof"]:
            b.write_field_vec(evals)
            b.write_merkle_proof(siblings)
        for step in rnd["steps"]:
            b.write_field_ext_vec(step["evals"])
            b.write_merkle_proof(step["merkle_proof"])
    b.write_field_ext_vec(fp["final_poly"])
    b.write_field(fp["pow_witness"])
    b.write_field_vec(proof["public_inputs"])
    return bytes(b.data)


def proof_from_bytes(data, desc, hasher=_lib.GL_HASHER_POSEIDON):
    """The proof dict: trace_cap, permutation_zs_cap (None without pairs), quotient_polys_cap, openings (permutation_zs /
    permutation_zs_next None without pairs), opening_proof as serialization.proof_from_bytes gives it, public_inputs."""
    fp = desc.fri_params
    h, perm = fp["cap_height"], bool(desc.pairs)
    b = Buffer(data, hasher)
    proof = dict(trace_cap=b.read_merkle_cap(h), permutation_zs_cap=b.read_merkle_cap(h) if perm else None, quotient_polys_cap=b.read_merkle_cap(h))
    proof["openings"] = dict(
        local_values=b.read_field_ext_vec(desc.num_columns), next_values=b.read_field_ext_vec(desc.num_columns),
        permutation_zs=b.read_field_ext_vec(desc.num_zs) if perm else None, permutation_zs_next=b.read_field_ext_vec(desc.num_zs) if perm else None,
        quotient_polys=b.read_field_ext_vec(desc.num_quotient_polys))
    caps = [b.read_merkle_cap(h) for _ in fp["reduction_arity_bits"]]
    leaf_lens = [desc.num_columns] + ([desc.num_zs] if perm else []) + [desc.num_quotient_polys]
    rounds = []
    for _ in range(fp["num_query_rounds"]):
        initial = []
        for n in leaf_lens:
            evals = b.read_field_vec(n)
            initial.append((evals, b.read_merkle_proof()))
        steps = []
        for ab in fp["reduction_arity_bits"]:
            evals = b.read_field_ext_vec(1 << ab)
            steps.append(dict(evals=evals, merkle_proof=b.read_merkle_proof()))
        rounds.append(dict(initial_trees_proof=initial, steps=steps))
    final = b.read_field_ext_vec(1 << (desc.degree_bits - sum(fp["reduction_arity_bits"])))
    pow_witness = b.read_field()
    proof["opening_proof"] = dict(commit_phase_merkle_caps=caps, query_round_proofs=rounds, final_poly=final, pow_witness=pow_witness)
    proof["public_inputs"] = b.read_field_vec(desc.num_public_inputs)
    if b.remaining():
        raise ValueError("IoError: %d bytes behind the proof" % b.remaining())
    return proof
