"""STARKs: starky's prove() on the device (gl_stark_create / gl_stark_prove, csrc/stark_prove.hip and csrc/stark.hip).

A STARK is described by its shape, its permutation pairs and ONE register program for all its constraints — what a host derives from
`Stark::eval_packed_generic` (starky/src/stark.rs) the way the gate programs are derived from `eval_unfiltered_*`. The program uses
the instruction set of gate_program.py with the STARK opcodes of include/plonky2_hip.h:

    LOAD_WIRE  dst <- local_values[a]          LOAD_NEXT dst <- next_values[a]          LOAD_PI dst <- public_inputs[a]
    EMIT            yield_constr.constraint(r[a])
    EMIT_TRANSITION yield_constr.constraint_transition(r[a])
    EMIT_FIRST_ROW  yield_constr.constraint_first_row(r[a])
    EMIT_LAST_ROW   yield_constr.constraint_last_row(r[a])

LOAD_CONST does not exist in a STARK program. The proof's wire format is defined in the header (the reference has no serializer for
StarkProofWithPublicInputs); proof_to_bytes / proof_from_bytes mirror it.

Several STARKs tied together by cross-table lookups (gl_stark_tables_create / gl_stark_tables_prove, the prover of the reference's
evm crate without anything EVM-specific) are a StarkTablesDesc: the tables' StarkDescs and a list of CrossTableLookup, each a list
of looking TableWithColumns and one looked TableWithColumns over CtlColumn linear combinations; NativeStarkTables is the handle,
tables_proof_to_bytes / tables_proof_from_bytes the wire format of its proofs."""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceBuffer
from .gate_program import ACC, ACCR, ADD, EMIT, LOAD_CONST, LOAD_IMM, LOAD_PI, LOAD_WIRE, MUL, MULK, SUB, GateAsm, ImmediatePool  # noqa: F401
from .serialization import Buffer
from .table import call_programs

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

    def eval_lookups(self, col_permuted_input, col_permuted_table):
        """eval_lookups (evm/src/lookup.rs:19-33): the constraints of one lookup whose permuted columns plonky2_gpu_amd.lookup
        fills. constraint_last_row of the next row's difference constrains the first row."""
        local_perm_input = self.local(col_permuted_input)
        next_perm_table = self.next(col_permuted_table)
        next_perm_input = self.next(col_permuted_input)
        diff_input_prev = self.sub(next_perm_input, local_perm_input)
        diff_input_table = self.sub(next_perm_input, next_perm_table)
        self.emit(self.mul(diff_input_prev, diff_input_table))
        self.emit_last_row(diff_input_table)

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


def _c_stark_desc(desc):
    """(GlStarkDesc, the arrays it points into: keep them alive for the call)"""
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
    return d, (arity, imms, flat, bounds, desc.instrs)


class NativeStark:
    """gl_stark_create: the handle of one STARK on one device; prove_bytes() = gl_stark_prove. `compiled`: compile(unit_instrs)
    at once."""

    def __init__(self, ctx, desc, hasher=_lib.GL_HASHER_POSEIDON, compiled=False, unit_instrs=None):
        self.ctx, self.desc, self.hasher = ctx, desc, _lib.hasher_id(hasher)
        self.ptr = None
        d, _keep = _c_stark_desc(desc)
        h = ctypes.c_void_p()
        _lib.call("gl_stark_create", self.hasher, ctypes.byref(d), ctypes.byref(h), ctx.ptr)
        self.ptr = h.value
        if compiled:
            self.compile(unit_instrs)

    def compile(self, unit_instrs=None):
        """gl_stark_compile: from now on the quotient runs the kernel generated from this STARK's description instead of the
        interpreter — the same values. Only between proofs; a second call is a no-op; on failure (Plonky2HipError with the
        compiler's log) the handle stays interpreted and usable. `unit_instrs` (gl_stark_compile_units): cut the description into
        kernels of at most that many instructions that run in order — what a long program needs to compile in reasonable time;
        0 takes the library's default cap, None is the single kernel."""
        if unit_instrs is None:
            _lib.call("gl_stark_compile", self.ptr, self.ctx.ptr)
        else:
            _lib.call("gl_stark_compile_units", self.ptr, int(unit_instrs), self.ctx.ptr)

    @property
    def is_compiled(self):
        return bool(_lib.load().gl_stark_is_compiled(self.ptr))

    @property
    def kernel_source(self):
        """the generated HIP source, or None unless compiled"""
        src = _lib.load().gl_stark_kernel_source(self.ptr)
        return None if src is None else src.decode()

    @property
    def num_units(self):
        """the number of kernels the quotient runs; 0 while interpreted"""
        return int(_lib.load().gl_stark_kernel_units(self.ptr))

    @property
    def unit_sources(self):
        """the generated HIP source of every unit in launch order, or None unless compiled"""
        if not self.is_compiled:
            return None
        return [_lib.load().gl_stark_kernel_unit_source(self.ptr, u).decode() for u in range(self.num_units)]

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
    _write_fri_proof(b, proof["opening_proof"])
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


# ---------------------------------------------------------------- cross-table lookups (evm/src/cross_table_lookup.rs)
class CtlColumn:
    """Column (cross_table_lookup.rs:29-119): sum_j coeff_j * row[col_j] + constant over the columns of one table. Coefficients and
    the constant are any integers, reduced mod p."""

    def __init__(self, terms=(), constant=0):
        self.terms = [(int(c), int(k) % P) for c, k in terms]
        self.constant = int(constant) % P

    @classmethod
    def single(cls, c):
        return cls([(c, 1)])

    @classmethod
    def linear_combination(cls, terms, constant=0):
        """`terms`: (column, coefficient) pairs"""
        return cls(terms, constant)

    @classmethod
    def constant(cls, k):  # shadowed per instance by the attribute of the same name
        return cls((), k)

    @classmethod
    def le_bits(cls, columns):
        """sum_j 2^j row[columns[j]]"""
        return cls([(c, 1 << j) for j, c in enumerate(columns)])

    @classmethod
    def sum(cls, columns):
        return cls([(c, 1) for c in columns])


class TableWithColumns:
    """TableWithColumns (:121-143): the columns of table number `table` that take part in a lookup and the filter that selects rows"""

    def __init__(self, table, columns, filter_column=None):
        self.table, self.columns, self.filter_column = int(table), list(columns), filter_column


class CrossTableLookup:
    """CrossTableLookup (:145-191). `default`: the row a verifier takes for the looking rows beyond the looked table's (only lookups
    without filters have one; the device never sees it)."""

    def __init__(self, looking_tables, looked_table, default=None):
        self.looking_tables, self.looked_table = list(looking_tables), looked_table
        self.default = None if default is None else [int(x) % P for x in default]
        twcs = self.twcs
        if any(len(t.columns) != len(looked_table.columns) for t in twcs):
            raise ValueError("the tables of a lookup have unequal numbers of columns")
        if len({t.filter_column is None for t in twcs}) > 1:
            raise ValueError("either every table of a lookup has a filter column or none has")
        if not self.looking_tables:
            raise ValueError("a lookup has at least one looking table")
        if default is not None and (twcs[0].filter_column is not None or len(self.default) != len(looked_table.columns)):
            raise ValueError("a default row belongs to a lookup without filters and has the lookup's number of columns")

    @property
    def twcs(self):
        """looking tables in order, then the looked table: the order of their CTL Zs under one challenge"""
        return self.looking_tables + [self.looked_table]


class StarkTablesDesc:
    """`tables`: StarkDescs (one StarkConfig: num_challenges and everything of fri_params but reduction_arity_bits agree; no public
    inputs), `lookups`: CrossTableLookups whose TableWithColumns name tables by their index."""

    def __init__(self, tables, lookups):
        self.tables, self.lookups = list(tables), list(lookups)

    @property
    def num_challenges(self):
        return self.tables[0].num_challenges

    def ctl_zs(self, table):
        """The CTL Zs of table number `table` in the order of cross_table_lookup_data (:237-312): (lookup, challenge, TWC)"""
        return [(li, c, t) for li, lk in enumerate(self.lookups) for c in range(self.num_challenges) for t in lk.twcs if t.table == table]

    def num_ctl_zs(self, table):
        return len(self.ctl_zs(table))

    def num_zs(self, table):
        """polynomials of the table's Zs oracle: permutation Zs, then CTL Zs"""
        return self.tables[table].num_zs + self.num_ctl_zs(table)

    def validate(self, hasher=_lib.GL_HASHER_POSEIDON):
        """What gl_stark_tables_create refuses about the shape (the constraint programs are checked by the library): ValueError"""
        keccak = _lib.hasher_id(hasher) == _lib.GL_HASHER_KECCAK25
        if not self.tables or not self.lookups:
            raise ValueError("No CTL? (no tables or no lookups)")
        shared = ("rate_bits", "cap_height", "proof_of_work_bits", "num_query_rounds")
        first = self.tables[0]
        for k, t in enumerate(self.tables):
            fp, where = t.fri_params, "table %d: " % k
            if fp.get("hiding"):
                raise ValueError(where + "a STARK's FRI parameters are not hiding")
            if not (1 <= t.degree_bits and t.degree_bits + fp["rate_bits"] <= 24 and 1 <= t.num_columns <= 65535 and 1 <= t.num_challenges <= 4
                    and t.constraint_degree >= 1):
                raise ValueError(where + "bad STARK shape")
            if t.quotient_degree_factor > 16 or t.quotient_degree_bits > fp["rate_bits"]:
                raise ValueError(where + "constraints of degree higher than the rate / quotient_degree_factor > 16")
            total = sum(fp["reduction_arity_bits"])
            if fp["cap_height"] > t.degree_bits + fp["rate_bits"] or total > t.degree_bits + fp["rate_bits"] - fp["cap_height"] or total > t.degree_bits:
                raise ValueError(where + "FRI total reduction arity is too large.")
            if any(c >= t.num_columns for pair in t.pairs for cp in pair for c in cp):
                raise ValueError(where + "permutation pair: column out of range")
            if t.num_challenges != first.num_challenges or any(fp[key] != first.fri_params[key] for key in shared):
                raise ValueError(where + "the tables share one StarkConfig; only reduction_arity_bits may differ")
            if t.num_public_inputs:
                raise ValueError(where + "a table of a multi-table STARK has no public inputs")
        for li, lk in enumerate(self.lookups):
            where = "lookup %d: " % li
            twcs = lk.twcs
            if len(twcs) < 2:
                raise ValueError(where + "a lookup has at least one looking table and the looked table")
            if any(len(t.columns) != len(twcs[0].columns) for t in twcs):
                raise ValueError(where + "its tables have unequal numbers of columns")
            if len({t.filter_column is None for t in twcs}) > 1:
                raise ValueError(where + "either every table of a lookup has a filter column or none has")
            for t in twcs:
                if not 0 <= t.table < len(self.tables):
                    raise ValueError(where + "table out of range")
                cols = t.columns + ([t.filter_column] if t.filter_column is not None else [])
                if any(not 0 <= c < self.tables[t.table].num_columns for col in cols for c, _ in col.terms):
                    raise ValueError(where + "a term's column is out of range for its table")
        for k, t in enumerate(self.tables):
            zs = self.ctl_zs(k)
            if not zs:
                raise ValueError("No CTL? (no lookup names table %d)" % k)
            need = 3 if any(tw.filter_column is not None for _, _, tw in zs) else 2
            if t.constraint_degree < need:
                raise ValueError("table %d: the checks of its CTL Zs have degree %d: constraint_degree must be at least that" % (k, need))
            if keccak:
                if 4 in (t.num_columns, self.num_zs(k), t.num_quotient_polys) or 1 in t.fri_params["reduction_arity_bits"]:
                    raise ValueError("table %d: KeccakHash<25> cannot hash a Merkle leaf of 4 elements" % k)

    def flatten(self):
        """The arrays of GlStarkTablesDesc: dict of numpy arrays. The CTL columns of a TWC are contiguous; filters come behind them."""
        term_columns, term_coeffs, column_bounds, constants = [], [], [0], []
        twc_table, twc_bounds, twc_filter, lookup_bounds = [], [0], [], [0]

        def add(col):
            term_columns.extend(c for c, _ in col.terms)
            term_coeffs.extend(k for _, k in col.terms)
            column_bounds.append(len(term_columns))
            constants.append(col.constant)
            return len(constants) - 1

        filters = []
        for lk in self.lookups:
            for t in lk.twcs:
                for col in t.columns:
                    add(col)
                twc_table.append(t.table)
                twc_bounds.append(len(constants))
                filters.append(t.filter_column)
            lookup_bounds.append(len(twc_table))
        for f in filters:
            twc_filter.append(_lib.GL_CTL_NO_FILTER if f is None else add(f))
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)  # noqa: E731
        return dict(term_columns=u32(term_columns), term_coeffs=_u64(term_coeffs), column_bounds=u32(column_bounds), column_constants=_u64(constants),
                    twc_table=u32(twc_table), twc_column_bounds=u32(twc_bounds), twc_filter=u32(twc_filter), lookup_bounds=u32(lookup_bounds))


def _tables_c_desc(desc, flat):
    """(GlStarkTablesDesc, keep-alive) from a StarkTablesDesc and its (possibly edited) flat arrays"""
    keep, structs = [flat], (_lib.GlStarkDesc * max(1, len(desc.tables)))()
    for k, t in enumerate(desc.tables):
        structs[k], alive = _c_stark_desc(t)
        keep.append(alive)
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    d = _lib.GlStarkTablesDesc(
        ctypes.sizeof(_lib.GlStarkTablesDesc), len(desc.tables), structs, ptr(flat["term_columns"]), ptr(flat["term_coeffs"]),
        flat["column_bounds"].ctypes.data, ptr(flat["column_constants"]), flat["column_constants"].size, ptr(flat["twc_table"]),
        flat["twc_column_bounds"].ctypes.data, ptr(flat["twc_filter"]), flat["twc_table"].size, flat["lookup_bounds"].ctypes.data,
        flat["lookup_bounds"].size - 1)
    return d, (keep, structs)


class NativeStarkTables:
    """gl_stark_tables_create: the handle of several STARKs and their cross-table lookups on one device. `flat`: the arrays of
    desc.flatten(), for callers that build them themselves. `compiled`: compile(unit_instrs) at once."""

    def __init__(self, ctx, desc, hasher=_lib.GL_HASHER_POSEIDON, flat=None, compiled=False, unit_instrs=None):
        self.ctx, self.desc, self.hasher = ctx, desc, _lib.hasher_id(hasher)
        self.ptr = None
        d, _keep = _tables_c_desc(desc, flat if flat is not None else desc.flatten())
        h = ctypes.c_void_p()
        _lib.call("gl_stark_tables_create", self.hasher, ctypes.byref(d), ctypes.byref(h), ctx.ptr)
        self.ptr = h.value
        if compiled:
            self.compile(unit_instrs)

    def compile(self, unit_instrs=None):
        """gl_stark_tables_compile: one generated quotient kernel per table (program, permutation checks and the table's CTL
        checks), as NativeStark.compile; all tables or none. `unit_instrs` (gl_stark_tables_compile_units): every table in units
        of at most that many instructions, 0 for the library's default cap."""
        if unit_instrs is None:
            _lib.call("gl_stark_tables_compile", self.ptr, self.ctx.ptr)
        else:
            _lib.call("gl_stark_tables_compile_units", self.ptr, int(unit_instrs), self.ctx.ptr)

    @property
    def is_compiled(self):
        return bool(_lib.load().gl_stark_tables_is_compiled(self.ptr))

    @property
    def kernel_source(self):
        """the generated HIP source per table, or None unless compiled"""
        if not self.is_compiled:
            return None
        return [_lib.load().gl_stark_tables_kernel_source(self.ptr, k).decode() for k in range(len(self.desc.tables))]

    @property
    def num_units(self):
        """per table the number of kernels its quotient runs; 0 while interpreted"""
        return [int(_lib.load().gl_stark_tables_kernel_units(self.ptr, k)) for k in range(len(self.desc.tables))]

    @property
    def unit_sources(self):
        """per table the generated HIP source of every unit in launch order, or None unless compiled"""
        if not self.is_compiled:
            return None
        return [[_lib.load().gl_stark_tables_kernel_unit_source(self.ptr, k, u).decode() for u in range(n)] for k, n in enumerate(self.num_units)]

    def prove_bytes(self, traces, timing=None, ctx=None):
        """`traces`: per table host [num_columns][n] value columns or a DeviceBuffer; `timing`: a list that receives one dict of stage
        times per table; `ctx`: another context of the handle's device (one proof per context at a time)."""
        ctx = ctx or self.ctx
        if len(traces) != len(self.desc.tables):
            raise ValueError("%d tables, %d traces" % (len(self.desc.tables), len(traces)))
        bufs = [t if isinstance(t, DeviceBuffer) else DeviceBuffer.from_host(ctx, _u64(t)) for t in traces]
        ptrs = (ctypes.c_void_p * len(bufs))(*[b.ptr for b in bufs])
        out, ln = ctypes.c_void_p(), ctypes.c_uint64()
        ms = np.zeros((len(bufs), _lib.GL_STARK_STAGES), dtype=np.float64) if timing is not None else None
        _lib.call("gl_stark_tables_prove", self.ptr, ctypes.addressof(ptrs), ctypes.byref(out), ctypes.byref(ln), ms, ctx.ptr)
        data = ctypes.string_at(out.value, ln.value)
        _lib.load().gl_bytes_free(out.value)
        if timing is not None:
            timing.extend({name: float(v) for name, v in zip(_lib.STARK_STAGE_NAMES, row)} for row in ms)
        return data

    def prove(self, traces, timing=None):
        return tables_proof_from_bytes(self.prove_bytes(traces, timing), self.desc, self.hasher)

    def ctl_zs(self, table, trace, ctl_challenges, trace_stride=None):
        """gl_stark_tables_ctl_zs. `trace`: host [num_columns][n] of table `table` (uploaded at pitch `trace_stride`, default n);
        `ctl_challenges`: num_challenges (beta, gamma). Returns [num_ctl_zs(table)][n]."""
        t = self.desc.tables[table]
        n = 1 << t.degree_bits
        stride = trace_stride or n
        host = np.zeros((t.num_columns, stride), dtype=np.uint64)
        host[:, :n] = _u64(trace)
        d_t = DeviceBuffer.from_host(self.ctx, host)
        nz = self.desc.num_ctl_zs(table)
        d_z = DeviceBuffer(self.ctx, nz * n)
        _lib.call("gl_stark_tables_ctl_zs", self.ptr, table, d_t.ptr, stride, _u64([w for bg in ctl_challenges for w in bg]), d_z.ptr, self.ctx.ptr)
        return d_z.download().reshape(nz, n)

    def quotient_polys(self, table, trace_lde, zs_lde, column_stride, alphas, challenge_sets, ctl_challenges):
        """gl_stark_tables_quotient_polys. `trace_lde` / `zs_lde`: DeviceBuffers (or pointers) of column-major LDEs at pitch
        `column_stride`, the Zs the permutation Zs then the CTL Zs; `challenge_sets` None without pairs. Returns the coefficients
        [num_challenges][n << quotient_degree_bits]."""
        t = self.desc.tables[table]
        size = 1 << (t.degree_bits + t.quotient_degree_bits)
        d_q = DeviceBuffer(self.ctx, t.num_challenges * size)
        ptr = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b  # noqa: E731
        ch = _challenge_words(challenge_sets) if challenge_sets is not None else None
        _lib.call("gl_stark_tables_quotient_polys", self.ptr, table, ptr(trace_lde), ptr(zs_lde), column_stride, _u64(alphas), ch,
                  _u64([w for bg in ctl_challenges for w in bg]), d_q.ptr, self.ctx.ptr)
        return d_q.download().reshape(t.num_challenges, size)

    def trim(self):
        _lib.call("gl_stark_tables_trim", self.ptr)

    def close(self):
        if self.ptr:
            _lib.load().gl_stark_tables_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def precompile(desc, hasher=_lib.GL_HASHER_POSEIDON, unit_instrs=None):
    """gl_stark_precompile / gl_stark_tables_precompile of a StarkDesc / StarkTablesDesc: validate as the handle's constructor
    does, generate the quotient kernel(s) and compile them into the kernel cache. Needs no device: what a build machine runs so
    that compile() finds its kernels. `unit_instrs` as compile()'s (gl_stark_precompile_units / gl_stark_tables_precompile_units)."""
    tables = isinstance(desc, StarkTablesDesc)
    d, _keep = _tables_c_desc(desc, desc.flatten()) if tables else _c_stark_desc(desc)
    name = "gl_stark_tables_precompile" if tables else "gl_stark_precompile"
    if unit_instrs is None:
        _lib.call(name, _lib.hasher_id(hasher), ctypes.byref(d))
    else:
        _lib.call(name + "_units", _lib.hasher_id(hasher), ctypes.byref(d), int(unit_instrs))


def split_program(desc, unit_instrs):
    """gl_stark_split_program: the unit programs compile(unit_instrs) cuts a StarkDesc's program into, as a list of
    (instrs [k][4] uint16, (first, one past the last) of the program's EMITs the unit yields). Every unit is a program of its own
    over desc.immediates; a value that lives across a cut is computed again in each unit that reads it. Needs no device."""
    d, _keep = _c_stark_desc(desc)
    instrs, gates, _, _ = call_programs("gl_stark_split_program", ctypes.byref(d), int(unit_instrs))
    return [(instrs[int(g[4]):int(g[4]) + int(g[5])], (int(g[2]), int(g[3]))) for g in gates]


# ---------------------------------------------------------------- wire format (include/plonky2_hip.h, gl_stark_tables_prove)
def _write_fri_proof(b, fp):
    """write_fri_proof (util/serialization.rs:591-639)"""
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


def tables_proof_to_bytes(proofs, desc, hasher=_lib.GL_HASHER_POSEIDON):
    """`proofs`: one StarkProof dict per table, as tables_proof_from_bytes gives them"""
    b = Buffer(hasher=hasher)
    for proof in proofs:
        for cap in ("trace_cap", "permutation_ctl_zs_cap", "quotient_polys_cap"):
            b.write_merkle_cap(proof[cap])
        op = proof["openings"]
        for key in ("local_values", "next_values", "permutation_ctl_zs", "permutation_ctl_zs_next"):
            b.write_field_ext_vec(op[key])
        b.write_field_vec(op["ctl_zs_last"])
        b.write_field_ext_vec(op["quotient_polys"])
        _write_fri_proof(b, proof["opening_proof"])
    return bytes(b.data)


def tables_proof_from_bytes(data, desc, hasher=_lib.GL_HASHER_POSEIDON):
    """One dict per table: trace_cap, permutation_ctl_zs_cap, quotient_polys_cap, openings (local_values, next_values,
    permutation_ctl_zs, permutation_ctl_zs_next, ctl_zs_last — base field elements —, quotient_polys), opening_proof."""
    b = Buffer(data, hasher)
    proofs = []
    for k, t in enumerate(desc.tables):
        fp = t.fri_params
        h, nz = fp["cap_height"], desc.num_zs(k)
        proof = dict(trace_cap=b.read_merkle_cap(h), permutation_ctl_zs_cap=b.read_merkle_cap(h), quotient_polys_cap=b.read_merkle_cap(h))
        proof["openings"] = dict(
            local_values=b.read_field_ext_vec(t.num_columns), next_values=b.read_field_ext_vec(t.num_columns),
            permutation_ctl_zs=b.read_field_ext_vec(nz), permutation_ctl_zs_next=b.read_field_ext_vec(nz),
            ctl_zs_last=b.read_field_vec(desc.num_ctl_zs(k)), quotient_polys=b.read_field_ext_vec(t.num_quotient_polys))
        caps = [b.read_merkle_cap(h) for _ in fp["reduction_arity_bits"]]
        rounds = []
        for _ in range(fp["num_query_rounds"]):
            initial = []
            for n in (t.num_columns, nz, t.num_quotient_polys):
                evals = b.read_field_vec(n)
                initial.append((evals, b.read_merkle_proof()))
            steps = []
            for ab in fp["reduction_arity_bits"]:
                evals = b.read_field_ext_vec(1 << ab)
                steps.append(dict(evals=evals, merkle_proof=b.read_merkle_proof()))
            rounds.append(dict(initial_trees_proof=initial, steps=steps))
        final = b.read_field_ext_vec(1 << (t.degree_bits - sum(fp["reduction_arity_bits"])))
        proof["opening_proof"] = dict(commit_phase_merkle_caps=caps, query_round_proofs=rounds, final_poly=final, pow_witness=b.read_field())
        proofs.append(proof)
    if b.remaining():
        raise ValueError("IoError: %d bytes behind the proofs" % b.remaining())
    return proofs
