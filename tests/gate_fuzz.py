"""A fixed, seeded list of gate tables for gl_compute_quotient_polys (TEST INFRASTRUCTURE ONLY): what tests/stark_fuzz.py is for the
STARK programs, for the plonk gate side — the interpreter of csrc/plonk.hip (eval_gate_program) and the kernel csrc/gate_jit.hip
generates, both against references that share no code with either.

Family A (A_CASES): gate LISTS drawn from CATALOG — all twenty gate kinds, every kind with parameters at two parameter sets or more —
in one to four selector groups, under one to four challenges, on 32 to 256 LDE points, at quotient degree factors 8, 4 (the kernel
reads half of the leaves), 3, 5, 6 and 7 (partial-product columns next to the gate terms). The programs are the emitters'
(plonky2_gpu_amd/gate_program.py); the reference is oracle/gates_ref.constraints under oracle/plonk_ref.evaluate_gate_constraints.

Family B (B_CASES): raw register PROGRAMS written by the generator below, not by the emitters: registers up to r63 and 45 live at
once, the four accumulators open together and one left open at the end of a gate, MULK by 0 / 32 / 63, ACC at the largest sum the
overflow contract allows on words whose halves are all ones, LOAD_IMM of zero, small, large and non-canonical constants as either
operand of ADD / SUB / MUL, the range-check pattern of the peephole pass (gate_jit.hip, rewrite 2) in its exact form and with one
condition broken, the same subexpression in two gates, one sum in two term orders, 256 constraints. The reference is the opcode
executor of tests/gate_exec.py under the same filter and Horner path.

Both references work on the RAW words: leaves, k_is, challenges and the public-inputs hash are uniform u64 with edge words sprinkled
in, nothing is reduced before it reaches the device.

fuzz_case(i) is entry i of CASES (family A first), fuzz_inputs(i, case) its inputs, reference_quotient(i) its expected output
(memoised: computed once per process); coverage() is what tests/test_gate_fuzz.py asserts about the list, so that a change of the
generator that loses a path fails on the CPU and not silently on the device."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gate_exec import execute  # noqa: E402
from oracle import gates_ref, plonk_ref, pyref  # noqa: E402
from plonky2_gpu_amd import gate_program as gp  # noqa: E402

P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
EDGES = (list(range(6)) + [(1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63] + [P + d for d in range(-4, 4)]
         + [M64 - 2, M64 - 1, M64])
EDGE_SHARES = [0.0, 0.03, 0.5]
RATE_BITS, ROUTED, SPARE_WIRES = 3, 8, 3
UNUSED_SELECTOR = 0xFFFFFFFF
SEED = 20270
KINDS_WITH_PARAMETERS = ["constant", "arithmetic", "base_sum", "comparison", "u32_add_many", "u32_arithmetic", "u32_subtraction", "u32_range_check",
                         "random_access", "arithmetic_extension", "mul_extension", "reducing", "reducing_extension", "exponentiation",
                         "low_degree_interpolation", "high_degree_interpolation"]
KINDS = KINDS_WITH_PARAMETERS + ["noop", "public_input", "poseidon_mds", "poseidon"]

# what tests/fuzz_gate_jit.py draws from (the Poseidon gate LAST: 4 000 operations, drawn now and then only) ...
CATALOG = [("noop", None), ("constant", 2), ("public_input", None), ("arithmetic", 3), ("arithmetic", 20), ("base_sum", (2, 7)), ("base_sum", (2, 63)),
           ("base_sum", (4, 16)), ("comparison", (8, 4)), ("comparison", (32, 16)), ("u32_add_many", (0, 2)), ("u32_add_many", (2, 3)),
           ("u32_add_many", (5, 2)), ("u32_add_many", (3, 4)), ("u32_arithmetic", 2), ("u32_arithmetic", 3), ("u32_subtraction", 3),
           ("u32_subtraction", 5), ("u32_range_check", 1), ("u32_range_check", 4), ("random_access", (2, 3, 2)), ("random_access", (4, 4, 2)),
           ("arithmetic_extension", 4), ("mul_extension", 5), ("reducing", 9), ("reducing_extension", 6), ("exponentiation", 13),
           ("poseidon_mds", None), ("low_degree_interpolation", 2), ("high_degree_interpolation", 2),
           # ... and further parameter sets of tests/test_gate_emit.CASES: the smallest ones, a base that is no power of two
           ("constant", 1), ("arithmetic", 1), ("base_sum", (3, 7)), ("comparison", (2, 1)), ("comparison", (10, 3)), ("random_access", (1, 2, 0)),
           ("random_access", (3, 1, 5)), ("low_degree_interpolation", 1), ("high_degree_interpolation", 1), ("high_degree_interpolation", 3),
           ("exponentiation", 1), ("reducing", 1), ("reducing_extension", 1), ("arithmetic_extension", 1), ("mul_extension", 2),
           ("u32_arithmetic", 1), ("u32_subtraction", 1),
           ("poseidon", None)]

# ---------------------------------------------------------------- family A: (gates or a number of gates to draw, selector groups,
# challenges, degree_bits, quotient_degree_factor)
A_CASES = [
    ([("arithmetic", 3), ("constant", 2), ("public_input", None), ("noop", None)], 1, 1, 2, 8),
    # the same gate twice: identical value graphs in one unit
    ([("base_sum", (2, 7)), ("base_sum", (3, 7)), ("u32_range_check", 1), ("u32_range_check", 1)], 2, 2, 3, 8),
    # 2, 3, 4: short, and between them the eight gate kinds of upstream plonky2 beyond the ed25519 list (LIFTED_A)
    ([("arithmetic_extension", 4), ("mul_extension", 5), ("reducing", 9)], 1, 3, 4, 4),
    ([("reducing_extension", 6), ("exponentiation", 13), ("poseidon_mds", None)], 3, 4, 2, 8),
    ([("low_degree_interpolation", 2), ("high_degree_interpolation", 2), ("reducing", 1), ("reducing_extension", 1), ("exponentiation", 1)], 2, 1, 3, 7),
    # gates without constraints and one real gate
    ([("noop", None), ("noop", None), ("noop", None), ("u32_subtraction", 3)], 2, 2, 5, 8),
    ([("comparison", (2, 1)), ("comparison", (10, 3)), ("random_access", (1, 2, 0)), ("random_access", (3, 1, 5))], 4, 3, 4, 4),
    # gates that range-check the same limbs: what fuse_partition puts together
    ([("u32_add_many", (0, 2)), ("u32_add_many", (2, 3)), ("u32_arithmetic", 2), ("u32_subtraction", 5), ("u32_range_check", 4)], 1, 2, 5, 8),
    # the one case with the Poseidon gate (its hiprtc time)
    ([("poseidon", None), ("arithmetic", 20), ("constant", 2)], 2, 2, 2, 8),
    # nine gates: more than one unit; quotient degree 3: two partial products per challenge
    ([("u32_add_many", (5, 2)), ("u32_add_many", (3, 4)), ("u32_arithmetic", 3), ("u32_subtraction", 3), ("u32_range_check", 1), ("base_sum", (4, 16)),
      ("comparison", (8, 4)), ("random_access", (2, 3, 2)), ("arithmetic", 3)], 3, 4, 3, 3),
    ([("low_degree_interpolation", 1), ("high_degree_interpolation", 1), ("high_degree_interpolation", 3), ("arithmetic_extension", 1),
      ("mul_extension", 2)], 2, 1, 4, 5),
    ([("base_sum", (2, 63)), ("comparison", (32, 16)), ("constant", 1), ("random_access", (4, 4, 2))], 3, 3, 2, 8),
    ([("exponentiation", 13), ("reducing", 9), ("reducing", 9), ("poseidon_mds", None), ("public_input", None)], 4, 4, 3, 8),
    ([("constant", 2), ("constant", 1), ("noop", None), ("arithmetic", 1), ("u32_arithmetic", 1), ("u32_subtraction", 1)], 1, 3, 5, 6),
    (7, 2, 2, 4, 8),
    (8, 4, 1, 5, 4),
]
LIFTED_A = [2, 3, 4]
POSEIDON_CASE = 8


def _groups(count, num_groups):
    assert 1 <= num_groups <= count
    cuts = [j * count // num_groups for j in range(num_groups + 1)]
    groups = [(cuts[j], cuts[j + 1]) for j in range(num_groups)]
    return groups, [j for j, (s, e) in enumerate(groups) for _ in range(s, e)]


def _finish(case, index, num_groups, num_challenges, degree_bits, qdf, ngc=None):
    programs = case["programs"]
    case["groups"], case["selector_indices"] = _groups(len(programs), num_groups)
    emits = [sum(1 for ins in p if ins[0] == gp.EMIT) for p in programs]
    case["num_gate_constraints"] = ngc if ngc is not None else max(1, max(emits))
    wires = 1 + max([ins[2] for p in programs for ins in p if ins[0] == gp.LOAD_WIRE] or [0])
    consts = 1 + max([ins[2] for p in programs for ins in p if ins[0] == gp.LOAD_CONST] or [0])
    case.update(index=index, seed=SEED + index, num_challenges=num_challenges, degree_bits=degree_bits, quotient_degree_factor=qdf,
                wires_loaded=wires, wires_len=max(ROUTED, wires) + SPARE_WIRES, num_constants=num_groups + consts,
                cs_len=num_groups + consts + ROUTED, qdb=(qdf - 1).bit_length(), num_prods=plonk_ref.num_partial_products(ROUTED, qdf))
    case["zs_len"] = num_challenges * (1 + case["num_prods"])
    case["n_ext"] = (1 << degree_bits) << RATE_BITS
    case["rows_read"] = (1 << degree_bits) << case["qdb"]  # the first n << qdb leaves hold the quotient domain
    assert 2 <= qdf and case["qdb"] <= RATE_BITS
    return case


def gate_list_case(gates, num_groups, num_challenges, degree_bits, qdf, index=0):
    """a family-A case of the given gates (tests/fuzz_gate_jit.py draws its own with this)"""
    pool = gp.ImmediatePool()
    programs = [gp.build_gate(kind, param, pool) for kind, param in gates]
    evaluators = [functools.partial(_oracle_gate, kind, param) for kind, param in gates]
    return _finish(dict(family="A", gates=list(gates), programs=programs, immediates=list(pool.values), evaluators=evaluators, ones_wires=[]),
                   index, num_groups, num_challenges, degree_bits, qdf)


def _case_a(i):
    gates, num_groups, nch, degree_bits, qdf = A_CASES[i]
    if isinstance(gates, int):
        rng = np.random.default_rng(SEED + i)
        gates = [CATALOG[int(rng.integers(0, len(CATALOG) - 1))] for _ in range(gates)]  # never the Poseidon gate
    return gate_list_case(gates, num_groups, nch, degree_bits, qdf, i)


def _oracle_gate(kind, param, consts, wires, pih):
    return gates_ref.constraints(kind, param, consts, wires, pih, gates_ref.Base)


# ---------------------------------------------------------------- family B: raw programs
IMM_VALUES = [0, 1, 2, 3, (1 << 32) - 1, 1 << 32, P - 1, P, P + 2, M64]
MULK_SHIFTS = [0, 32, 63]
ACC_MAX = 1 << 31  # 2^31 (2^32 - 1) < 2^63 <= (2^31 + 1) (2^32 - 1): the largest sum of weights one accumulation may hold
# the range-check pattern t = a b; u = t + 2; c = t u; EMIT c (gate_jit.hip, rewrite 2: "with t, u, c read nowhere else") and what is planted
# next to it. REWRITABLE are the forms that ARE the pattern for a pass that follows values and not spellings: the operands of the
# commutative ADD and MUL in either order, the constant as any representative of 2, a = b. In the others one condition is broken.
REWRITABLE = ("exact", "two_plus_t", "u_times_t", "p_plus_2", "a_equals_b")
NEAR_MISSES = ("t_read_later", "u_read_later", "c_read_later", "c_emitted_twice", "constant_1", "constant_3")
FILLER_WEIGHTS = {gp.LOAD_WIRE: 10, gp.LOAD_CONST: 4, gp.LOAD_PI: 4, gp.LOAD_IMM: 6, gp.ADD: 9, gp.SUB: 9, gp.MUL: 10, gp.MULK: 6, gp.ACC: 9, gp.ACCR: 5,
                  gp.EMIT: 5}
FILLER_ACC_WEIGHTS = [0, 1, 3, (1 << 30) - 1, 1 << 31, (1 << 32) - 1]  # 2^32 - 1 never fits; 2^31 fits alone


class _Table:
    """what the gates of one family-B case share: the immediates (NOT reduced and not deduplicated by value mod p: p and 0 are two
    entries), the wire columns handed out so far, the columns that hold the all-ones word, the labels of what was planted"""

    def __init__(self):
        self.imms, self.next_wire, self.ones_wires, self.planted, self.programs = [], ROUTED, [], [], []

    def imm(self, v):
        assert 0 <= v <= M64
        if v not in self.imms:
            self.imms.append(v)
        return self.imms.index(v)

    def wire(self):
        self.next_wire += 1
        return self.next_wire - 1

    def gate(self):
        g = _Gate(self, len(self.programs))
        self.programs.append(g.ins)
        return g


class _Gate:
    """one gate's program, valid by construction: every method asserts the rule it could break. `readable`: the registers the random
    filler may read — the temporaries of a planted pattern are not among them (a later read would break the pattern)."""

    def __init__(self, table, row):
        self.t, self.row, self.ins = table, row, []
        self.written, self.readable = set(), []
        self.bound, self.opened = [0] * 4, [False] * 4

    def _put(self, op, dst, a, b, reads=(), writes=True, share=True):
        assert all(0 <= r < gp.MAX_REGS and r in self.written for r in reads), "a register is written before it is read"
        assert 0 <= dst < gp.MAX_REGS and 0 <= a < 65536 and 0 <= b < 65536
        self.ins.append((op, dst, a, b))
        if writes:
            self.written.add(dst)
            if share and dst not in self.readable:
                self.readable.append(dst)
            if not share and dst in self.readable:
                self.readable.remove(dst)
        return dst

    def wire(self, dst, col=None, share=True):
        return self._put(gp.LOAD_WIRE, dst, self.t.wire() if col is None else col, 0, share=share)

    def const(self, dst, col):
        return self._put(gp.LOAD_CONST, dst, col, 0)

    def pi(self, dst, k):
        assert k < 4
        return self._put(gp.LOAD_PI, dst, k, 0)

    def imm(self, dst, v, share=True):
        return self._put(gp.LOAD_IMM, dst, self.t.imm(v), 0, share=share)

    def alu(self, op, dst, a, b, share=True):
        assert op in (gp.ADD, gp.SUB, gp.MUL)
        return self._put(op, dst, a, b, reads=(a, b), share=share)

    def mulk(self, dst, a, shift):
        assert shift < 64
        return self._put(gp.MULK, dst, a, shift, reads=(a,))

    def acc(self, q, a, weight):
        assert q < 4 and weight < 1 << 32 and self.bound[q] + weight * 0xFFFFFFFF < gp.ACC_LIMIT
        self.bound[q] += weight * 0xFFFFFFFF
        self.opened[q] = True
        self._put(gp.ACC, q, a, self.t.imm(weight), reads=(a,), writes=False)

    def accr(self, dst, q):
        assert q < 4 and self.opened[q], "an ACCR comes only after an ACC on that accumulator"
        self.bound[q], self.opened[q] = 0, False
        return self._put(gp.ACCR, dst, q, 0)

    def emit(self, a):
        self._put(gp.EMIT, 0, a, 0, reads=(a,), writes=False)

    @property
    def emits(self):
        return sum(1 for ins in self.ins if ins[0] == gp.EMIT)

    def label(self, what, **more):
        self.t.planted.append(dict(more, what=what, gate=self.row))

    # ---- what is planted
    def pattern(self, variant):
        """r0 .. r6 are its temporaries; fresh wire columns, so that no two planted patterns are one value"""
        assert variant in REWRITABLE + NEAR_MISSES
        self.wire(0, share=False)
        b = 0 if variant == "a_equals_b" else self.wire(1, share=False)
        two = {"constant_1": 1, "constant_3": 3, "p_plus_2": P + 2}.get(variant, 2)
        self.imm(2, two, share=False)
        self.alu(gp.MUL, 3, 0, b, share=False)  # t
        self.alu(gp.ADD, 4, *((2, 3) if variant == "two_plus_t" else (3, 2)), share=False)  # u
        self.alu(gp.MUL, 5, *((4, 3) if variant == "u_times_t" else (3, 4)), share=False)  # c
        self.emit(5)
        if variant.endswith("_read_later"):
            self.alu(gp.ADD, 6, {"t": 3, "u": 4, "c": 5}[variant[0]], 0, share=False)
            self.emit(6)
        if variant == "c_emitted_twice":
            self.emit(5)
        self.label("pattern", variant=variant, rewritable=variant in REWRITABLE)

    def immediates(self, values, ops=(gp.ADD, gp.SUB, gp.MUL)):
        """x (op) K and K (op) x for every K: rewrites 1 and 3 with the constant in either position"""
        for v in values:
            for op in ops:
                self.wire(0)
                self.imm(1, v, share=False)
                self.emit(self.alu(op, 2, 0, 1))
                self.emit(self.alu(op, 3, 1, 0))

    def immediate_that_stays(self, v):
        """one LOAD_IMM read by a foldable ADD and by readers that take a register: MULK, ACC, EMIT"""
        self.wire(0)
        self.imm(1, v, share=False)
        self.emit(self.alu(gp.ADD, 2, 0, 1))
        self.emit(self.mulk(3, 1, 5))
        self.acc(0, 1, 3)
        self.emit(self.accr(4, 0))
        self.emit(1)
        self.label("immediate_that_stays", value=v)

    def high_registers(self):
        for r in (60, 61, 62, 63):
            self.wire(r)
        self.alu(gp.ADD, 63, 60, 61)
        self.alu(gp.MUL, 62, 62, 63)
        self.alu(gp.SUB, 61, 62, 60)
        self.emit(61)
        self.emit(63)

    def many_live(self, count=45):
        for r in range(count):
            self.wire(r)
        for r in range(1, count):  # r0 <- ((r0 + r1) r2 - r3 + r4) r5 ...
            self.alu((gp.ADD, gp.MUL, gp.SUB)[(r - 1) % 3], 0, 0, r)
        self.emit(0)

    def four_accumulators(self):
        regs = [self.wire(r) for r in range(4)]
        for rnd in range(3):
            for q in range(4):
                self.acc(q, regs[(q + rnd) % 4], [1, 3, 1 << 20, (1 << 28) + 5][(q + 2 * rnd) % 4])
        for q in range(4):
            self.accr(8 + q, q)
        self.alu(gp.ADD, 12, 8, 9)
        self.alu(gp.MUL, 13, 10, 11)
        self.emit(self.alu(gp.SUB, 14, 12, 13))
        self.label("four_accumulators_open")

    def leave_accumulator_open(self, q=2):
        """the LAST thing of a gate; the next gate's start_from_zero() reads the same accumulator"""
        self.acc(q, self.wire(0), 12345)
        self.acc(q, self.wire(1, col=self.t.ones_wire()), 1 << 30)
        self.label("accumulator_left_open", q=q)

    def start_from_zero(self, q=2):
        assert not self.ins
        self.acc(q, self.wire(0), 1)
        self.emit(self.accr(1, q))  # = the wire, whatever the gate before left
        self.label("accumulator_starts_from_zero", q=q)

    def mulk_shifts(self):
        for s in MULK_SHIFTS:
            self.wire(0)
            self.emit(self.mulk(1, 0, s))

    def acc_bounds(self):
        ones = self.wire(0, col=self.t.ones_wire())
        self.acc(0, ones, ACC_MAX)  # 2^31 alone
        self.emit(self.accr(1, 0))
        other = self.wire(2)
        for j in range(32):  # 32 terms of 2^26: the same bound over many terms
            self.acc(1, ones if j % 4 else other, 1 << 26)
        assert self.bound[1] == ACC_MAX * 0xFFFFFFFF
        self.emit(self.accr(3, 1))
        self.acc(0, ones, ACC_MAX)  # an ACCR starts the bound again
        self.accr(4, 0)
        self.acc(0, ones, ACC_MAX - 1)
        self.acc(0, other, 1)
        self.accr(5, 0)
        self.emit(self.alu(gp.SUB, 6, 4, 5))
        self.label("acc_bounds")

    def shared_subexpression(self, cols):
        """(w0 w1 + w2) (w0 - w2) over the given columns: planted in two gates of a case"""
        for r, c in enumerate(cols):
            self.wire(r, col=c)
        self.alu(gp.MUL, 3, 0, 1)
        self.alu(gp.ADD, 3, 3, 2)
        self.alu(gp.SUB, 4, 0, 2)
        self.emit(self.alu(gp.MUL, 5, 3, 4))
        self.label("shared_subexpression", columns=list(cols))

    def weighted_sum(self, cols, order):
        """sum of w_j * (3, 5, 7, 5)[j] with the ACCs in the given order: one term multiset, two orders in two gates"""
        for r, c in enumerate(cols):
            self.wire(r, col=c)
        for j in order:
            self.acc(3, j, (3, 5, 7, 5)[j])
        self.emit(self.accr(7, 3))
        self.label("weighted_sum", columns=list(cols), order=list(order))

    def filler(self, rng, length, max_emits):
        """random valid instructions, as tests/stark_fuzz.gen_program draws them. It loads no representative of 2, so that it cannot
        complete the peephole pattern by chance: the rewrites of a case are the planted ones."""
        end = len(self.ins) + length
        while len(self.ins) < end:
            ops = [op for op in FILLER_WEIGHTS if not (op == gp.ACCR and not any(self.opened)) and not (op == gp.EMIT and self.emits >= max_emits)]
            if not self.readable:
                ops = [gp.LOAD_WIRE, gp.LOAD_CONST, gp.LOAD_PI]
            w = np.array([FILLER_WEIGHTS[op] for op in ops], dtype=np.float64)
            op = ops[int(rng.choice(len(ops), p=w / w.sum()))]
            src = lambda: self.readable[int(rng.integers(0, len(self.readable)))]  # noqa: E731

            def dst(sources=()):
                u = rng.random()
                if sources and u < 0.15:
                    return sources[int(rng.integers(0, len(sources)))]  # ADD r, r, x
                if u < 0.30:
                    return int(rng.integers(56, 64))
                if self.readable and u < 0.50:
                    return src()  # overwritten after use
                return int(rng.integers(0, gp.MAX_REGS))

            if op == gp.LOAD_WIRE:
                self.wire(dst(), col=int(rng.integers(0, self.t.next_wire)))
            elif op == gp.LOAD_CONST:
                self.const(dst(), int(rng.integers(0, 3)))
            elif op == gp.LOAD_PI:
                self.pi(dst(), int(rng.integers(0, 4)))
            elif op == gp.LOAD_IMM:
                v = IMM_VALUES[int(rng.integers(0, len(IMM_VALUES)))] if rng.random() < 0.5 else int(rng.integers(0, M64, dtype=np.uint64, endpoint=True))
                self.imm(dst(), v if v % P != 2 else 5)
            elif op in (gp.ADD, gp.SUB, gp.MUL):
                a = src()
                b = a if rng.random() < 0.1 else src()
                self.alu(op, dst((a, b)), a, b)
            elif op == gp.MULK:
                a = src()
                self.mulk(dst((a,)), a, MULK_SHIFTS[int(rng.integers(0, 3))] if rng.random() < 0.6 else int(rng.integers(0, 64)))
            elif op == gp.ACC:
                q = int(rng.integers(0, 4))
                fits = [k for k in FILLER_ACC_WEIGHTS if self.bound[q] + k * 0xFFFFFFFF < gp.ACC_LIMIT]  # 0 always fits
                self.acc(q, src(), fits[int(rng.integers(0, len(fits)))])
            elif op == gp.ACCR:
                open_ = [q for q in range(4) if self.opened[q]]
                self.accr(dst(), open_[int(rng.integers(0, len(open_)))])
            else:
                self.emit(src())

    def close(self):
        """reduce what the filler left open and emit it, so that the gate's last value is checked"""
        for q in range(4):
            if self.opened[q]:
                self.emit(self.accr(q, q))


def _ones_wire(table):
    table.ones_wires.append(table.wire())
    return table.ones_wires[-1]


_Table.ones_wire = _ones_wire


def _b0(t, rng):
    """one gate of 8 instructions: the exact pattern and one more load, in a table of its own"""
    g = t.gate()
    g.pattern("exact")
    g.wire(9)
    assert len(g.ins) == 8


def _b1(t, rng):
    """the pattern in every form, rewritable and not, in two gates"""
    g = t.gate()
    for v in ("exact", "t_read_later", "two_plus_t", "constant_1", "u_read_later", "a_equals_b", "c_emitted_twice"):
        g.pattern(v)
    h = t.gate()
    for v in ("constant_3", "exact", "c_read_later", "p_plus_2", "u_times_t"):
        h.pattern(v)


def _b2(t, rng):
    """every constant as either operand of ADD, SUB and MUL; constants whose load has to stay"""
    g = t.gate()
    g.immediates(IMM_VALUES)
    for v in (2, P + 2, M64, 1 << 32):
        g.immediate_that_stays(v)
    g.filler(rng, 40, 100)
    g.close()


def _b3(t, rng):
    """registers: r60 .. r63, 45 live at once, the four accumulators open together, one left open across a gate boundary, MULK"""
    g = t.gate()
    g.high_registers()
    g.many_live()
    g.four_accumulators()
    g.mulk_shifts()
    g.leave_accumulator_open()
    h = t.gate()
    h.start_from_zero()
    h.filler(rng, 60, 4)
    h.close()


def _b4(t, rng):
    """ACC at its bound on all-ones words; one sum in two orders and one subexpression in two gates"""
    cols = [t.wire() for _ in range(4)]
    g = t.gate()
    g.acc_bounds()
    g.weighted_sum(cols, (0, 1, 2, 3))
    g.shared_subexpression(cols[:3])
    h = t.gate()
    h.shared_subexpression(cols[:3])
    h.weighted_sum(cols, (2, 3, 0, 1))
    h.pattern("exact")
    k = t.gate()
    k.weighted_sum(cols, (3, 1, 0, 2))
    k.mulk_shifts()


def _b5(t, rng):
    """num_gate_constraints = 256 (GP_MAX_CONSTRAINTS): one gate emits all of them, the other fewer"""
    g = t.gate()
    g.wire(1)
    for k in range(256):
        g.wire(0, col=k % t.next_wire)
        g.emit(g.alu((gp.ADD, gp.MUL, gp.SUB)[k % 3], 1, 1, 0))
    h = t.gate()
    h.filler(rng, 50, 7)
    h.close()


def _filler_gates(lengths, max_emits=12):
    def build(t, rng):
        for n in lengths:
            g = t.gate()
            g.filler(rng, n, max_emits)
            g.close()
    return build


def _b8(t, rng):
    """the planted things among random instructions"""
    g = t.gate()
    g.filler(rng, 80, 6)
    g.pattern("exact")
    g.filler(rng, 80, 12)
    g.pattern("c_read_later")
    g.immediates([0, 3, P, M64], ops=(gp.SUB,))
    g.close()
    h = t.gate()
    h.filler(rng, 100, 8)
    h.mulk_shifts()
    h.pattern("p_plus_2")
    h.close()


def _b9(t, rng):
    g = t.gate()
    g.high_registers()
    g.filler(rng, 150, 10)
    g.immediate_that_stays(0)
    g.close()
    t.gate().filler(rng, 8, 0)  # a gate that emits nothing (the filler closes no accumulator here: they may stay open)


# (builder, selector groups, challenges, degree_bits, quotient_degree_factor, num_gate_constraints or None: the largest number a gate emits)
B_CASES = [
    (_b0, 1, 2, 3, 8, None),
    (_b1, 2, 2, 4, 8, None),
    (_b2, 1, 1, 3, 8, 120),  # the gate emits fewer than num_gate_constraints
    (_b3, 2, 3, 4, 4, None),
    (_b4, 3, 4, 3, 8, None),
    (_b5, 2, 2, 2, 8, 256),
    (_filler_gates([600, 200, 60, 8]), 4, 1, 5, 8, None),
    (_filler_gates([300, 120, 30]), 2, 3, 2, 7, None),
    (_b8, 2, 4, 5, 4, None),
    (_b9, 1, 2, 2, 3, None),
]
LIFTED_B = [1, 2]  # indices into B_CASES
SUMS_CASE = 4  # the family-B case whose sums are all over wires: one sum in three term orders, one sum twice
NEAR_MISS_CASES = [1, 8]  # family-B cases whose rewrite count the GPU test asserts (1: every form)
LIMIT_CASE = 5


def _case_b(j):
    build, num_groups, nch, degree_bits, qdf, ngc = B_CASES[j]
    t = _Table()
    build(t, np.random.default_rng(SEED + 1000 + j))
    programs = [list(p) for p in t.programs]
    evaluators = [functools.partial(_execute_gate, p, t.imms) for p in programs]
    return _finish(dict(family="B", gates=["raw program of %d instructions" % len(p) for p in programs], programs=programs, immediates=list(t.imms),
                        evaluators=evaluators, ones_wires=list(t.ones_wires), planted=t.planted),
                   len(A_CASES) + j, num_groups, nch, degree_bits, qdf, ngc)


def _execute_gate(program, imms, consts, wires, pih):
    return execute(program, imms, 0, consts, wires, pih, open_accumulators=True)


CASES = list(range(len(A_CASES) + len(B_CASES)))
FAMILY_B = CASES[len(A_CASES):]


@functools.lru_cache(maxsize=None)
def fuzz_case(i):
    return _case_a(i) if i < len(A_CASES) else _case_b(i - len(A_CASES))


def describe(case):
    return dict(seed=case["seed"], family=case["family"], gates=case["gates"], groups=case["groups"], challenges=case["num_challenges"],
                degree_bits=case["degree_bits"], quotient_degree_factor=case["quotient_degree_factor"], constraints=case["num_gate_constraints"])


# ---------------------------------------------------------------- inputs
def draw_leaves(rng, shape, share):
    """uniform u64 words with a share of EDGES among them"""
    x = rng.integers(0, M64, size=shape, dtype=np.uint64, endpoint=True)
    edge = np.array(EDGES, dtype=np.uint64)[rng.integers(0, len(EDGES), size=shape)]
    return np.where(rng.random(shape) < share, edge, x)


def draw_inputs(rng, case, share):
    """everything gl_compute_quotient_polys reads, as raw words: leaf-major leaves [n_ext][leaf_len] of the three commitments, k_is, the
    challenges, the public-inputs hash. About half of the rows carry honest selector words — the index of one gate of the table in its
    group's column, UNUSED_SELECTOR in the others — so that every other gate's filter is seen to vanish there."""
    n_ext, groups = case["n_ext"], case["groups"]
    wires = draw_leaves(rng, (n_ext, case["wires_len"]), share)
    cs = draw_leaves(rng, (n_ext, case["cs_len"]), share)
    zs = draw_leaves(rng, (n_ext, case["zs_len"]), share)
    for col in case["ones_wires"]:
        wires[:, col] = np.where(rng.random(n_ext) < 0.75, np.uint64(M64), wires[:, col])
    honest = np.flatnonzero(rng.random(n_ext) < 0.5)
    rows = rng.integers(0, len(case["programs"]), size=honest.size)
    for g in range(len(groups)):
        mine = np.array([case["selector_indices"][r] == g for r in rows], dtype=bool)
        cs[honest, g] = np.where(mine, rows.astype(np.uint64), np.uint64(UNUSED_SELECTOR))
    u64 = lambda count: [int(v) for v in rng.integers(0, M64, size=count, dtype=np.uint64, endpoint=True)]  # noqa: E731
    nch = case["num_challenges"]
    return dict(wires=wires, cs=cs, zs=zs, k_is=np.array(u64(ROUTED), dtype=np.uint64), alphas=u64(nch), betas=u64(nch), gammas=u64(nch), pih=u64(4))


@functools.lru_cache(maxsize=None)
def _inputs(i):
    return draw_inputs(np.random.default_rng(7 * SEED + i), fuzz_case(i), EDGE_SHARES[(i + 2 * (i in FAMILY_B)) % 3])


def fuzz_inputs(i, case=None):
    """the inputs of case i (`case` is accepted for symmetry with tests/stark_fuzz.py); the arrays are shared: do not write to them"""
    return _inputs(i)


# ---------------------------------------------------------------- references
def gate_terms(case, inp):
    """evaluate_gate_constraints at every point of the quotient domain, in the domain's order: [n << qdb][num_gate_constraints]"""
    bits, step = case["degree_bits"] + RATE_BITS, 1 << (RATE_BITS - case["qdb"])
    wires, cs = inp["wires"].tolist(), inp["cs"].tolist()
    out = []
    for i in range(case["rows_read"]):
        row = pyref.reverse_bits(i * step, bits)
        out.append(plonk_ref.evaluate_gate_constraints(case["evaluators"], case["selector_indices"], case["groups"], case["num_gate_constraints"],
                                                       cs[row], wires[row], inp["pih"]))
    return out


def quotient_of(case, inp):
    """plonk_ref.compute_quotient_polys over gate_terms, on the raw words -> canonical uint64 [num_challenges][n << qdb]"""
    out = plonk_ref.compute_quotient_polys(inp["wires"].tolist(), inp["cs"].tolist(), inp["zs"].tolist(), case["num_constants"],
                                           [int(k) for k in inp["k_is"]], inp["betas"], inp["gammas"], inp["alphas"], case["degree_bits"], RATE_BITS,
                                           case["quotient_degree_factor"], gate_terms(case, inp))
    return np.array([[int(v) % P for v in col] for col in out], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def reference_quotient(i):
    return quotient_of(fuzz_case(i), fuzz_inputs(i))


# ---------------------------------------------------------------- the validity rules, restated (include/plonky2_hip.h)
def validate(programs, immediates, num_gate_constraints):
    """raises ValueError at the first instruction that breaks a rule of the gate-program encoding"""
    for g, prog in enumerate(programs):
        written, bound, opened, emits = set(), [0] * 4, [False] * 4, 0
        for pc, (op, dst, a, b) in enumerate(prog):
            where = "gate %d instruction %d" % (g, pc)
            if not 0 <= op <= gp.ACCR:
                raise ValueError(where + ": unknown opcode")
            reads = [a, b] if op in (gp.ADD, gp.SUB, gp.MUL) else [a] if op in (gp.EMIT, gp.MULK, gp.ACC) else []
            if any(r >= gp.MAX_REGS for r in reads) or (op not in (gp.EMIT, gp.ACC) and dst >= gp.MAX_REGS):
                raise ValueError(where + ": register index out of range")
            if any(r not in written for r in reads):
                raise ValueError(where + ": register read before any write")
            if op == gp.LOAD_PI and a >= 4:
                raise ValueError(where + ": LOAD_PI index out of range")
            if op == gp.LOAD_IMM and a >= len(immediates):
                raise ValueError(where + ": LOAD_IMM index out of range")
            if op == gp.MULK and b >= 64:
                raise ValueError(where + ": MULK shift out of range")
            if op == gp.ACC:
                if dst >= 4 or b >= len(immediates) or immediates[b] >= 1 << 32:
                    raise ValueError(where + ": ACC accumulator or immediate out of range")
                bound[dst] += immediates[b] * 0xFFFFFFFF
                opened[dst] = True
                if bound[dst] >= 1 << 63:
                    raise ValueError(where + ": the accumulator could reach 2^63")
            if op == gp.ACCR:
                if a >= 4 or not opened[a]:
                    raise ValueError(where + ": ACCR of an accumulator nothing was added to")
                bound[a], opened[a] = 0, False
            if op == gp.EMIT:
                emits += 1
            elif op != gp.ACC:
                written.add(dst)
        if emits > min(num_gate_constraints, 256):
            raise ValueError("gate %d emits %d constraints" % (g, emits))


# ---------------------------------------------------------------- what the list reaches
def _reaching(prog):
    """per instruction: the instruction that wrote operand a / operand b (None: not a register read)"""
    last, out = {}, []
    for op, dst, a, b in prog:
        ra = last.get(a) if op in (gp.ADD, gp.SUB, gp.MUL, gp.EMIT, gp.MULK, gp.ACC) else None
        rb = last.get(b) if op in (gp.ADD, gp.SUB, gp.MUL) else None
        out.append((ra, rb))
        if op not in (gp.EMIT, gp.ACC):
            last[dst] = len(out) - 1
    return out


def _max_live(prog):
    live, most = set(), 0
    for op, dst, a, b in reversed(prog):
        if op not in (gp.EMIT, gp.ACC):
            live.discard(dst)
        if op in (gp.ADD, gp.SUB, gp.MUL):
            live.update((a, b))
        elif op in (gp.EMIT, gp.MULK, gp.ACC):
            live.add(a)
        most = max(most, len(live))
    return most


def program_coverage(case):
    """what the raw programs of one family-B case reach, read off the instructions (and, for what is a matter of intent, off the
    generator's labels)"""
    imms = case["immediates"]
    c = dict(ops=set(), high_registers=set(), max_live=0, accumulators_open=0, open_at_gate_end=False, mulk_shifts=set(), acc_single_max=False,
             acc_many_terms_max=False, acc_restart=False, imm_operands=set(), imm_kept=set(), fewer_emits=False, gates_without_emit=0)
    for prog in case["programs"]:
        reach = _reaching(prog)
        opened, bound, terms, reduced = [False] * 4, [0] * 4, [0] * 4, [False] * 4
        emits = 0
        c["max_live"] = max(c["max_live"], _max_live(prog))
        for pc, (op, dst, a, b) in enumerate(prog):
            c["ops"].add(op)
            regs = ([a, b] if op in (gp.ADD, gp.SUB, gp.MUL) else [a] if op in (gp.EMIT, gp.MULK, gp.ACC) else []) + ([dst] if op not in (gp.EMIT, gp.ACC) else [])
            c["high_registers"].update(r for r in regs if r >= 60)
            for pos, d in enumerate(reach[pc]):
                if d is not None and prog[d][0] == gp.LOAD_IMM:
                    if op in (gp.ADD, gp.SUB, gp.MUL):
                        c["imm_operands"].add((op, pos, imms[prog[d][2]]))
                    else:
                        c["imm_kept"].add(imms[prog[d][2]])
            if op == gp.MULK:
                c["mulk_shifts"].add(b)
            elif op == gp.ACC:
                opened[dst], bound[dst], terms[dst] = True, bound[dst] + imms[b] * 0xFFFFFFFF, terms[dst] + 1
                c["accumulators_open"] = max(c["accumulators_open"], sum(opened))
            elif op == gp.ACCR:
                at_max = bound[a] == ACC_MAX * 0xFFFFFFFF
                c["acc_single_max"] |= at_max and terms[a] == 1
                c["acc_many_terms_max"] |= at_max and terms[a] >= 16
                c["acc_restart"] |= at_max and reduced[a]
                opened[a], bound[a], terms[a], reduced[a] = False, 0, 0, True
            elif op == gp.EMIT:
                emits += 1
        c["open_at_gate_end"] |= any(opened)
        c["fewer_emits"] |= 0 < emits < case["num_gate_constraints"]
        c["gates_without_emit"] += emits == 0
    return c


def coverage():
    """what CASES reaches; tests/test_gate_fuzz.py asserts it"""
    a = [fuzz_case(i) for i in CASES if fuzz_case(i)["family"] == "A"]
    b = [fuzz_case(i) for i in FAMILY_B]
    parameters = {}
    for case in a:
        for kind, param in case["gates"]:
            parameters.setdefault(kind, set()).add(param)
    every = a + b
    cov = dict(
        parameters=parameters,
        groups={len(c["groups"]) for c in every}, challenges={c["num_challenges"] for c in every}, degree_bits={c["degree_bits"] for c in every},
        quotient_degree_factors=[c["quotient_degree_factor"] for c in a],
        poseidon_cases=[c["index"] for c in a if ("poseidon", None) in c["gates"]],
        partial_products=any(c["num_prods"] > 0 for c in a),
        duplicate_gates=any(c["gates"].count(g) > 1 and gates_ref.num_constraints(*g) > 0 for c in a for g in c["gates"]),
        one_real_gate=any(sum(1 for g in c["gates"] if gates_ref.num_constraints(*g)) == 1 and len(c["gates"]) >= 3 for c in a),
        spare_wires=all(c["wires_len"] >= c["wires_loaded"] + SPARE_WIRES for c in every),
        gates_per_case=sorted(len(c["gates"]) for c in a),
        program_lengths=sorted(len(p) for c in b for p in c["programs"]),
        max_constraints=max(c["num_gate_constraints"] for c in b),
        emits_256=any(sum(1 for ins in p if ins[0] == gp.EMIT) == 256 for c in b for p in c["programs"]),
        planted=[dict(p, case=c["index"]) for c in b for p in c["planted"]],
    )
    per = [program_coverage(c) for c in b]
    for key in ("ops", "high_registers", "mulk_shifts", "imm_operands", "imm_kept"):
        cov[key] = set().union(*(p[key] for p in per))
    for key in ("max_live", "accumulators_open"):
        cov[key] = max(p[key] for p in per)
    for key in ("open_at_gate_end", "acc_single_max", "acc_many_terms_max", "acc_restart", "fewer_emits"):
        cov[key] = any(p[key] for p in per)
    return cov


def distinct_wire_sums(case):
    """how many different sums the ACCRs of a case reduce, a sum being the multiset of its (wire column, weight) terms whatever their
    order — what a generator that shares values across gates keeps one accumulator for. Only for cases whose ACC terms are all wires."""
    sums = set()
    for prog in case["programs"]:
        reach, terms = _reaching(prog), [[] for _ in range(4)]
        for pc, (op, dst, a, b) in enumerate(prog):
            if op == gp.ACC:
                load = prog[reach[pc][0]]
                assert load[0] == gp.LOAD_WIRE, "a term that is no wire"
                terms[dst].append((load[2], case["immediates"][b]))
            elif op == gp.ACCR:
                sums.add(tuple(sorted(terms[a])))
                terms[a] = []
    return len(sums)


def planted_rewrites(case):
    """how many of the case's planted patterns the peephole pass has to rewrite"""
    return sum(1 for p in case["planted"] if p["what"] == "pattern" and p["rewritable"])
