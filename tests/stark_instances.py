"""Three STARKs and one family of STARKs as data (TEST INFRASTRUCTURE): shape, permutation pairs, the constraint program in the encoding of
include/plonky2_hip.h (assembled with plonky2_gpu_amd.stark.StarkAsm), the same constraints as a hand-written closure over a field
object (tests/stark_ref.py Base / Ext), and a trace generator.

A  the reference's FibonacciStark (starky/src/fibonacci_stark.rs): 4 columns, 3 public inputs, degree 2 (qdf 1, qdb 0), one
   permutation pair singletons(2, 3).
B  5 columns, degree 3 (qdf 2, qdb 1), 2 public inputs, a program that uses every opcode, three permutation pairs — one with two
   column pairs — so that num_pairs * num_challenges is odd for 1 and 3 challenges: several batches, the last one short.
C  5 columns, degree 4 (qdf 3, qdb 2: the chunk copy and the tail check of a quotient_degree_factor that is no power of two),
   3 public inputs, no permutation pairs.
D(d)  the family of constraint degree d = 2 .. 17 (qdf d - 1 up to the library's limit of 16): 4 columns, one public input,
   c0' = c0 + 1, c1' = c1^(d-1) c0 + K, c0 starts at pi[0]; columns 2 and 3 hold the rows (c0, c1) under one permutation, pairs
   [[(0, 2), (1, 3)], [(2, 0)]]: with at most 4 challenges never more than 8 instances, so one short batch from qdf 8 on.
   D(d, public_input=False) starts c0 at an immediate instead: no public inputs at all. D(d, columns=5) has a fifth column
   c4' = c4 + c0, for the Keccak hasher, which cannot hash leaves of 4 elements.

Degrees: a constraint of degree d in the columns leaves a quotient of degree < (d - 1) n as a transition (times z_last) or on all
rows; behind a Lagrange selector it may have degree d - 1 at most."""
import numpy as np

from plonky2_gpu_amd.stark import StarkAsm, StarkDesc

P = 0xFFFFFFFF00000001


class TestStark:
    __test__ = False  # not a pytest class

    def __init__(self, name, num_columns, num_public_inputs, constraint_degree, pairs, asm, closure, make_trace):
        self.name, self.num_columns, self.num_public_inputs, self.constraint_degree = name, num_columns, num_public_inputs, constraint_degree
        self.pairs, self.closure, self.make_trace = pairs, closure, make_trace
        self.instrs, self.immediates = asm.program()

    def desc(self, degree_bits, num_challenges, fri_params):
        return StarkDesc(degree_bits, self.num_columns, self.num_public_inputs, self.constraint_degree, num_challenges, fri_params, self.instrs,
                         self.immediates, self.pairs)


def fri_params(rate_bits=1, cap_height=0, arity_bits=(), num_query_rounds=5, proof_of_work_bits=3):
    return dict(rate_bits=rate_bits, cap_height=cap_height, proof_of_work_bits=proof_of_work_bits, num_query_rounds=num_query_rounds,
                reduction_arity_bits=list(arity_bits), hiding=False)


# ---------------------------------------------------------------- A: FibonacciStark
def _fib_program():
    a = StarkAsm()
    a.emit_first_row(a.sub(a.local(0), a.pi(0)))
    a.emit_first_row(a.sub(a.local(1), a.pi(1)))
    a.emit_last_row(a.sub(a.local(1), a.pi(2)))
    a.release()
    a.emit_transition(a.sub(a.next(0), a.local(1)))  # x0' <- x1
    a.emit_transition(a.sub(a.sub(a.next(1), a.local(0)), a.local(1)))  # x1' <- x0 + x1
    return a


def _fib_closure(F, local, nxt, pis, c):  # fibonacci_stark.rs:64-86
    c.constraint_first_row(F.sub(local[0], pis[0]))
    c.constraint_first_row(F.sub(local[1], pis[1]))
    c.constraint_last_row(F.sub(local[1], pis[2]))
    c.constraint_transition(F.sub(nxt[0], local[1]))
    c.constraint_transition(F.sub(F.sub(nxt[1], local[0]), local[1]))


def _fib_trace(degree_bits, seed=0):
    """generate_trace (fibonacci_stark.rs:44-57) from (x0, x1) = (seed, 1); returns (columns, public inputs)"""
    n = 1 << degree_bits
    rows, acc = [], [seed % P, 1, 0, 1]
    for _ in range(n):
        rows.append(list(acc))
        acc = [acc[1], (acc[0] + acc[1]) % P, acc[2] + 1, acc[3] + 1]
    rows[n - 1][3] = 0  # so that columns 2 and 3 are permutations of one another
    return [[r[k] for r in rows] for k in range(4)], [rows[0][0], rows[0][1], rows[n - 1][1]]


A = TestStark("A", 4, 3, 2, [[(2, 3)]], _fib_program(), _fib_closure, _fib_trace)

# ---------------------------------------------------------------- B: degree 3, every opcode, three pairs
B_K = 0x123456789ABCDEF  # an immediate above 2^32


def _b_program():
    a = StarkAsm()
    c0, c1, c2 = a.local(0), a.local(1), a.local(2)
    a.emit_first_row(a.sub(c0, a.pi(0)))  # the counter starts at pi[0] ...
    a.emit_last_row(a.sub(c0, a.pi(1)))  # ... and ends at pi[1]
    a.emit_transition(a.sub(a.next(0), a.add(c0, a.imm(1))))  # c0' = c0 + 1
    a.emit_transition(a.sub(a.sub(a.next(1), a.mul(a.mul(c1, c1), c0)), a.imm(B_K)))  # c1' = c1^2 c0 + K: degree 3
    # c2 = 3 c0 + 7 c1 + 2^5 c0 on every row: ACC / ACCR and MULK
    a.acc(c0, 3)
    a.acc(c1, 7)
    a.emit(a.sub(a.sub(c2, a.accr()), a.mulk(c0, 5)))
    return a


def _b_closure(F, local, nxt, pis, c):
    c.constraint_first_row(F.sub(local[0], pis[0]))
    c.constraint_last_row(F.sub(local[0], pis[1]))
    c.constraint_transition(F.sub(nxt[0], F.add(local[0], F.one)))
    c.constraint_transition(F.sub(F.sub(nxt[1], F.mul(F.mul(local[1], local[1]), local[0])), F.lift(B_K)))
    weighted = F.add(F.mul(local[0], F.lift(35)), F.mul(local[1], F.lift(7)))
    c.constraint(F.sub(local[2], weighted))


def _b_trace(degree_bits, seed=0):
    n = 1 << degree_bits
    start = 1000 + seed
    c0 = [(start + r) % P for r in range(n)]
    c1 = [(seed * 77 + 5) % P]
    for r in range(n - 1):
        c1.append((c1[r] * c1[r] % P * c0[r] + B_K) % P)
    c2 = [(35 * x + 7 * y) % P for x, y in zip(c0, c1)]
    sigma = np.random.default_rng(seed + 11).permutation(n)
    c3, c4 = [c0[s] for s in sigma], [c2[s] for s in sigma]  # the rows (c0, c2) permuted together
    return [c0, c1, c2, c3, c4], [c0[0], c0[n - 1]]


B = TestStark("B", 5, 2, 3, [[(0, 3), (2, 4)], [(3, 0)], [(4, 2)]], _b_program(), _b_closure, _b_trace)


# ---------------------------------------------------------------- C: degree 4, no pairs
def _c_program():
    a = StarkAsm()
    c0, c1, c2, c3, c4 = (a.local(k) for k in range(5))
    a.emit_first_row(a.sub(c0, a.pi(0)))
    a.emit_first_row(a.sub(c3, a.pi(1)))
    a.emit_last_row(a.sub(c4, a.pi(2)))
    a.emit_transition(a.sub(a.next(0), a.add(c0, a.imm(1))))  # c0' = c0 + 1
    a.emit_transition(a.sub(a.sub(a.next(1), a.mul(a.mul(a.mul(c1, c1), c1), c0)), c2))  # c1' = c1^3 c0 + c2: degree 4
    a.emit_transition(a.sub(a.sub(a.next(2), c2), a.mul(c3, c4)))  # c2' = c2 + c3 c4
    a.emit_transition(a.sub(a.next(3), c4))  # c3' = c4
    a.emit_transition(a.sub(a.sub(a.next(4), c3), c4))  # c4' = c3 + c4
    return a


def _c_closure(F, local, nxt, pis, c):
    c.constraint_first_row(F.sub(local[0], pis[0]))
    c.constraint_first_row(F.sub(local[3], pis[1]))
    c.constraint_last_row(F.sub(local[4], pis[2]))
    c.constraint_transition(F.sub(nxt[0], F.add(local[0], F.one)))
    cube = F.mul(F.mul(local[1], local[1]), local[1])
    c.constraint_transition(F.sub(F.sub(nxt[1], F.mul(cube, local[0])), local[2]))
    c.constraint_transition(F.sub(F.sub(nxt[2], local[2]), F.mul(local[3], local[4])))
    c.constraint_transition(F.sub(nxt[3], local[4]))
    c.constraint_transition(F.sub(F.sub(nxt[4], local[3]), local[4]))


def _c_trace(degree_bits, seed=0):
    n = 1 << degree_bits
    rows, acc = [], [(7 + seed) % P, (3 + seed) % P, 11, (2 + seed) % P, 1]
    for _ in range(n):
        rows.append(list(acc))
        c0, c1, c2, c3, c4 = acc
        acc = [(c0 + 1) % P, (pow(c1, 3, P) * c0 + c2) % P, (c2 + c3 * c4) % P, c4, (c3 + c4) % P]
    return [[r[k] for r in rows] for k in range(5)], [rows[0][0], rows[0][3], rows[n - 1][4]]


C = TestStark("C", 5, 3, 4, [], _c_program(), _c_closure, _c_trace)



# ---------------------------------------------------------------- D(d): degree d, qdf = d - 1
D_K = 0xFEDCBA9876543  # an immediate above 2^32
D_START = 77  # where c0 starts without a public input


def D(d, public_input=True, columns=4):
    assert 2 <= d <= 17 and columns in (4, 5)

    def program():
        a = StarkAsm()
        c0, c1 = a.local(0), a.local(1)
        a.emit_first_row(a.sub(c0, a.pi(0) if public_input else a.imm(D_START)))
        a.emit_transition(a.sub(a.next(0), a.add(c0, a.imm(1))))  # c0' = c0 + 1
        power = c1
        for _ in range(d - 2):
            power = a.mul(power, c1)
        a.emit_transition(a.sub(a.sub(a.next(1), a.mul(power, c0)), a.imm(D_K)))  # c1' = c1^(d-1) c0 + K: degree d
        if columns == 5:
            a.emit_transition(a.sub(a.sub(a.next(4), a.local(4)), c0))  # c4' = c4 + c0
        return a

    def closure(F, local, nxt, pis, c):
        c.constraint_first_row(F.sub(local[0], pis[0] if public_input else F.lift(D_START)))
        c.constraint_transition(F.sub(nxt[0], F.add(local[0], F.one)))
        power = local[1]
        for _ in range(d - 2):
            power = F.mul(power, local[1])
        c.constraint_transition(F.sub(F.sub(nxt[1], F.mul(power, local[0])), F.lift(D_K)))
        if columns == 5:
            c.constraint_transition(F.sub(F.sub(nxt[4], local[4]), local[0]))

    def make_trace(degree_bits, seed=0):
        n = 1 << degree_bits
        start = 500 + seed if public_input else D_START
        c0 = [(start + r) % P for r in range(n)]
        c1 = [(seed * 31 + 3) % P]
        for r in range(n - 1):
            c1.append((pow(c1[r], d - 1, P) * c0[r] + D_K) % P)
        sigma = np.random.default_rng(seed + 17).permutation(n)
        cols = [c0, c1, [c0[s] for s in sigma], [c1[s] for s in sigma]]  # the rows (c0, c1) permuted together
        if columns == 5:
            c4 = [(seed + 9) % P]
            for r in range(n - 1):
                c4.append((c4[r] + c0[r]) % P)
            cols.append(c4)
        return cols, [c0[0]] if public_input else []

    name = "D%d%s%s" % (d, "" if public_input else "n", "" if columns == 4 else "k")
    return TestStark(name, columns, int(public_input), d, [[(0, 2), (1, 3)], [(2, 0)]], program(), closure, make_trace)


# D at the degrees the tests use: qdf 4 (one full batch at 2 challenges), 5 (no power of two: chunk copy, batches 5 + 1), 8, 16 (the
# limit); "n": no public inputs; "k": five columns
STARKS = {"A": A, "B": B, "C": C}
STARKS.update({s.name: s for s in (D(5), D(6), D(9), D(17), D(5, public_input=False), D(5, columns=5), D(17, columns=5))})
