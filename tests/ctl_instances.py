"""One system of three STARK tables tied by three cross-table lookups, as data (TEST INFRASTRUCTURE), and a family of random
descriptions for the CTL quotient. For every table: shape, permutation pairs, the constraint program (plonky2_gpu_amd.stark.StarkAsm), the
same constraints as a hand-written closure, and the table's CTL checks written out by hand (tests/ctl_ref.py takes both).

    table 0  "ops"    2^3 rows, 7 columns, no pairs:   c0 counter from START, c1' = c1^2 c0 + K (degree 3), c2 / c3 two disjoint binary
                                                       flags, c4 c5 c6 bits
    table 1  "rows"   2^3 rows, 5 columns, no pairs:   t0 t1 a looked tuple, t2 a binary padding flag, t3 free, t4 counter from START
    table 2  "small"  2^2 rows, 5 columns, one pair:   u0 free, u1 a permutation of u0 (pair [(0, 1)]), u2 counter, u3' = u3^2 u2 + K,
                                                       u4 = u0 + u2

    lookup 0  filtered.  looking: table 0 (le_bits(c4, c5, c6), constant 7) where c2 = 1   — a le_bits column with coefficients 2^j, a
                                                                                             constant-only column
                         looking: table 0 (c1, c0 + 3) where c2 + c3 = 1                   — the same table a second time; a filter that
                                                                                             is a sum of two columns
                         looked:  table 1 (t0, t1) where 1 - t2 = 1                        — a filter with a constant
    lookup 1  no filters, default (DEFAULT,): looking table 1 (t3), 8 rows; looked table 2 (u0), 4 rows — unequal heights: the four
              other rows of t3 hold DEFAULT. Table 1 is looked in lookup 0 and looking here.
    lookup 2  no filters, no default: looking table 0 (c0), looked table 1 (t4), the two counters.

system(constraint_degree): every table declares that degree (3 is what the constraints need; 4 gives quotient_degree_factor 3,
which no power of two and, with two challenges, no Keccak leaf of 4). The traces satisfy every constraint and every lookup;
check_traces asserts that row by row."""
import numpy as np

from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, StarkAsm, StarkDesc, StarkTablesDesc, TableWithColumns

import ctl_ref as cr
import stark_ref as sr

P = 0xFFFFFFFF00000001
START, K, DEFAULT = 40, 0x123456789ABCDEF, 0xDEFA017
DEGREE_BITS = (3, 3, 2)
ARITY_BITS = ((2,), (2,), ())  # per table: reduction_arity_bits may differ


class Table:
    def __init__(self, name, num_columns, constraint_degree, pairs, asm, closure):
        self.name, self.num_columns, self.num_public_inputs, self.constraint_degree = name, num_columns, 0, constraint_degree
        self.pairs, self.closure = pairs, closure
        self.instrs, self.immediates = asm.program()


class System:
    def __init__(self, tables, lookups, ctl_closures):
        self.tables, self.lookups, self.ctl_closures = tables, lookups, ctl_closures

    def desc(self, degree_bits, num_challenges, fri_params):
        """StarkTablesDesc; `fri_params`: one dict per table"""
        return StarkTablesDesc([StarkDesc(db, t.num_columns, 0, t.constraint_degree, num_challenges, fp, t.instrs, t.immediates, t.pairs)
                                for t, db, fp in zip(self.tables, degree_bits, fri_params)], self.lookups)


def fri_params(rate_bits=1, cap_height=0, arity_bits=ARITY_BITS, num_query_rounds=4, proof_of_work_bits=2):
    """one dict per table"""
    return [dict(rate_bits=rate_bits, cap_height=cap_height, proof_of_work_bits=proof_of_work_bits, num_query_rounds=num_query_rounds,
                 reduction_arity_bits=list(ab), hiding=False) for ab in arity_bits]


# ---------------------------------------------------------------- the tables' own constraints
def _binary(a, x):
    a.emit(a.mul(x, a.sub(x, a.imm(1))))


def _ops_program():
    a = StarkAsm()
    c0, c1, c2, c3 = (a.local(k) for k in range(4))
    a.emit_first_row(a.sub(c0, a.imm(START)))
    a.emit_transition(a.sub(a.next(0), a.add(c0, a.imm(1))))
    a.emit_transition(a.sub(a.sub(a.next(1), a.mul(a.mul(c1, c1), c0)), a.imm(K)))
    _binary(a, c2)
    _binary(a, c3)
    a.emit(a.mul(c2, c3))
    for k in (4, 5, 6):
        _binary(a, a.local(k))
    return a


def _ops_closure(F, l, n, pis, c):
    one = F.one
    c.constraint_first_row(F.sub(l[0], F.lift(START)))
    c.constraint_transition(F.sub(n[0], F.add(l[0], one)))
    c.constraint_transition(F.sub(F.sub(n[1], F.mul(F.mul(l[1], l[1]), l[0])), F.lift(K)))
    c.constraint(F.mul(l[2], F.sub(l[2], one)))
    c.constraint(F.mul(l[3], F.sub(l[3], one)))
    c.constraint(F.mul(l[2], l[3]))
    for k in (4, 5, 6):
        c.constraint(F.mul(l[k], F.sub(l[k], one)))


def _rows_program():
    a = StarkAsm()
    _binary(a, a.local(2))
    a.emit_first_row(a.sub(a.local(4), a.imm(START)))
    a.emit_transition(a.sub(a.next(4), a.add(a.local(4), a.imm(1))))
    return a


def _rows_closure(F, l, n, pis, c):
    c.constraint(F.mul(l[2], F.sub(l[2], F.one)))
    c.constraint_first_row(F.sub(l[4], F.lift(START)))
    c.constraint_transition(F.sub(n[4], F.add(l[4], F.one)))


def _small_program():
    a = StarkAsm()
    u0, u2, u3 = a.local(0), a.local(2), a.local(3)
    a.emit_transition(a.sub(a.next(2), a.add(u2, a.imm(1))))
    a.emit_transition(a.sub(a.sub(a.next(3), a.mul(a.mul(u3, u3), u2)), a.imm(K)))
    a.emit(a.sub(a.sub(a.local(4), u0), u2))
    return a


def _small_closure(F, l, n, pis, c):
    c.constraint_transition(F.sub(n[2], F.add(l[2], F.one)))
    c.constraint_transition(F.sub(F.sub(n[3], F.mul(F.mul(l[3], l[3]), l[2])), F.lift(K)))
    c.constraint(F.sub(F.sub(l[4], l[0]), l[2]))


# ---------------------------------------------------------------- the CTL checks by hand
def _checks(F, c, z, z_next, value, value_next, filt=None, filt_next=None):
    """the two constraints of one CTL Z from its closed-form row value and filter"""
    def select(f, x):
        return x if f is None else F.sub(F.add(F.mul(f, x), F.one), f)

    c.constraint_first_row(F.sub(z, select(filt, value)))
    c.constraint_transition(F.sub(z_next, F.mul(z, select(filt_next, value_next))))


def _ops_ctl(F, l, n, zs, zs_next, challenges, c):
    """table 0: per challenge the two looking TWCs of lookup 0, then per challenge the looking TWC of lookup 2"""
    L, k = F.lift, 0
    for beta, gamma in challenges:
        bits = lambda r: F.add(F.add(r[4], F.mul(r[5], L(2))), F.mul(r[6], L(4)))  # noqa: E731
        a = lambda r: F.add(F.add(bits(r), F.mul(L(beta), L(7))), L(gamma))  # noqa: E731
        _checks(F, c, zs[k], zs_next[k], a(l), a(n), l[2], n[2])
        b = lambda r: F.add(F.add(r[1], F.mul(L(beta), F.add(r[0], L(3)))), L(gamma))  # noqa: E731
        _checks(F, c, zs[k + 1], zs_next[k + 1], b(l), b(n), F.add(l[2], l[3]), F.add(n[2], n[3]))
        k += 2
    for beta, gamma in challenges:
        _checks(F, c, zs[k], zs_next[k], F.add(l[0], L(gamma)), F.add(n[0], L(gamma)))
        k += 1


def _rows_ctl(F, l, n, zs, zs_next, challenges, c):
    """table 1: looked in lookup 0, looking in lookup 1, looked in lookup 2"""
    L, k = F.lift, 0
    for beta, gamma in challenges:
        v = lambda r: F.add(F.add(r[0], F.mul(L(beta), r[1])), L(gamma))  # noqa: E731
        _checks(F, c, zs[k], zs_next[k], v(l), v(n), F.sub(F.one, l[2]), F.sub(F.one, n[2]))
        k += 1
    for col in (3, 4):
        for beta, gamma in challenges:
            _checks(F, c, zs[k], zs_next[k], F.add(l[col], L(gamma)), F.add(n[col], L(gamma)))
            k += 1


def _small_ctl(F, l, n, zs, zs_next, challenges, c):
    """table 2: looked in lookup 1"""
    for k, (beta, gamma) in enumerate(challenges):
        _checks(F, c, zs[k], zs_next[k], F.add(l[0], F.lift(gamma)), F.add(n[0], F.lift(gamma)))


OPS_A = TableWithColumns(0, [CtlColumn.le_bits([4, 5, 6]), CtlColumn.constant(7)], CtlColumn.single(2))
OPS_B = TableWithColumns(0, [CtlColumn.single(1), CtlColumn.linear_combination([(0, 1)], 3)], CtlColumn.sum([2, 3]))
ROWS_LOOKED = TableWithColumns(1, [CtlColumn.single(0), CtlColumn.single(1)], CtlColumn.linear_combination([(2, P - 1)], 1))
LOOKUPS = [CrossTableLookup([OPS_A, OPS_B], ROWS_LOOKED),
           CrossTableLookup([TableWithColumns(1, [CtlColumn.single(3)])], TableWithColumns(2, [CtlColumn.single(0)]), default=[DEFAULT]),
           CrossTableLookup([TableWithColumns(0, [CtlColumn.single(0)])], TableWithColumns(1, [CtlColumn.single(4)]))]


def system(constraint_degree=3):
    tables = [Table("ops", 7, constraint_degree, [], _ops_program(), _ops_closure),
              Table("rows", 5, constraint_degree, [], _rows_program(), _rows_closure),
              Table("small", 5, constraint_degree, [[(0, 1)]], _small_program(), _small_closure)]
    return System(tables, LOOKUPS, [_ops_ctl, _rows_ctl, _small_ctl])


# the CTL Zs of every table with two challenges, written out by hand: (lookup, challenge, which TWC)
ZS_ORDER_2 = [
    [(0, 0, OPS_A), (0, 0, OPS_B), (0, 1, OPS_A), (0, 1, OPS_B), (2, 0, LOOKUPS[2].looking_tables[0]), (2, 1, LOOKUPS[2].looking_tables[0])],
    [(0, 0, ROWS_LOOKED), (0, 1, ROWS_LOOKED), (1, 0, LOOKUPS[1].looking_tables[0]), (1, 1, LOOKUPS[1].looking_tables[0]),
     (2, 0, LOOKUPS[2].looked_table), (2, 1, LOOKUPS[2].looked_table)],
    [(1, 0, LOOKUPS[1].looked_table), (1, 1, LOOKUPS[1].looked_table)],
]


def make_traces(seed=0):
    """[table][column][row] values that satisfy everything"""
    rng = np.random.default_rng(900 + seed)
    word = lambda: int(rng.integers(0, P, dtype=np.uint64))  # noqa: E731
    n0, n1, n2 = (1 << db for db in DEGREE_BITS)
    c0 = [START + r for r in range(n0)]
    c1 = [(5 + seed) % P]
    for r in range(n0 - 1):
        c1.append((c1[r] * c1[r] % P * c0[r] + K) % P)
    c2 = [1 if r in (1, 4) else 0 for r in range(n0)]
    c3 = [1 if r in (2, 5, 6) else 0 for r in range(n0)]
    bits = [[int(rng.integers(0, 2)) for _ in range(n0)] for _ in range(3)]
    ops = [c0, c1, c2, c3] + bits
    tuples = [(bits[0][r] + 2 * bits[1][r] + 4 * bits[2][r], 7) for r in range(n0) if c2[r]]
    tuples += [(c1[r], c0[r] + 3) for r in range(n0) if c2[r] + c3[r]]
    assert len(tuples) == 7 and n1 == 8
    looked = [(t, 0) for t in tuples] + [((word(), word()), 1)]  # one padding row, its tuple arbitrary
    looked = [looked[i] for i in rng.permutation(n1)]
    u0 = [word() for _ in range(n2)]
    t3 = u0 + [DEFAULT] * (n1 - n2)
    t3 = [t3[i] for i in rng.permutation(n1)]
    rows = [[t[0] for t, _ in looked], [t[1] for t, _ in looked], [pad for _, pad in looked], t3, [START + r for r in range(n1)]]
    u2 = [(3 + seed + r) % P for r in range(n2)]
    u3 = [9]
    for r in range(n2 - 1):
        u3.append((u3[r] * u3[r] % P * u2[r] + K) % P)
    small = [u0, [u0[i] for i in rng.permutation(n2)], u2, u3, [(a + b) % P for a, b in zip(u0, u2)]]
    return [ops, rows, small]


def check_traces(sys_, traces, challenge=(0x1234567, 0x89ABCDEF)):
    """every constraint of every table on every row (first / last / transition where they apply), and the product identity of every
    lookup under one challenge: AssertionError otherwise"""
    for stark, trace in zip(sys_.tables, traces):
        n = len(trace[0])
        for r in range(n):
            local, nxt = [col[r] for col in trace], [col[(r + 1) % n] for col in trace]
            # on the subgroup: z_last vanishes on the last row only, the Lagrange selectors are 1 on their row and 0 elsewhere
            consumer = sr.Consumer(sr.Base, [1], 0 if r == n - 1 else 1, 1 if r == 0 else 0, 1 if r == n - 1 else 0)
            sr.eval_constraints(sr.Base, stark, local, nxt, [], consumer, "closure")
            assert all(e == 0 for e in consumer.emitted), (stark.name, "row", r, consumer.emitted)
    assert cr.product_identity_holds(sys_.lookups, traces, challenge)
    return True


# ---------------------------------------------------------------- random descriptions for the quotient alone
class RandomSystem:
    """two tables: table 0 carries a random program, 0 - 2 permutation pairs and `appearances` looking TWCs (one lookup each, random
    columns of 1 - 5 CTL columns, with or without filter); table 1 is the looked side of every lookup. Only the quotient of table 0
    is run, on random words: nothing has to hold."""

    def __init__(self, seed, qdf, degree_bits, appearances, num_pairs, num_challenges):
        import stark_fuzz as sf

        rng = np.random.default_rng(31000 + seed)
        self.degree_bits, self.num_challenges, self.rate_bits = degree_bits, num_challenges, max(1, (qdf - 1).bit_length())
        num_columns = int(rng.integers(2, 9))
        pairs = [[(int(rng.integers(0, num_columns)), int(rng.integers(0, num_columns))) for _ in range(int(rng.integers(1, 3)))]
                 for _ in range(num_pairs)]
        instrs, immediates = sf.gen_program(rng, num_columns, 0, 40)
        t0 = sf.FuzzStark(num_columns, 0, qdf + 1, pairs, instrs, immediates)
        a = StarkAsm()
        a.emit(a.local(0))
        i1, m1 = a.program()
        t1 = sf.FuzzStark(6, 0, 3, [], i1, m1)
        self.tables = [t0, t1]

        def column(ncols):
            terms = [(int(rng.integers(0, ncols)), int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))) for _ in range(int(rng.integers(0, 4)))]
            return CtlColumn(terms, int(rng.integers(0, P, dtype=np.uint64)) if rng.random() < 0.5 else 0)

        self.lookups, self.widths = [], []
        for _ in range(appearances):
            width, filtered = int(rng.integers(1, 6)), bool(rng.integers(0, 2))
            self.widths.append(width)
            self.lookups.append(CrossTableLookup([TableWithColumns(0, [column(num_columns) for _ in range(width)], column(num_columns) if filtered else None)],
                                                 TableWithColumns(1, [column(6) for _ in range(width)], column(6) if filtered else None)))
        self.ctl_closures = None

    def desc(self):
        fp = dict(rate_bits=self.rate_bits, cap_height=0, proof_of_work_bits=0, num_query_rounds=1, reduction_arity_bits=[], hiding=False)
        mk = lambda t, db: StarkDesc(db, t.num_columns, 0, t.constraint_degree, self.num_challenges, fp, t.instrs, t.immediates, t.pairs)  # noqa: E731
        return StarkTablesDesc([mk(self.tables[0], self.degree_bits), mk(self.tables[1], 1)], self.lookups)


# (qdf, degree_bits, appearances, pairs, challenges): CTL Zs of table 0 = appearances * challenges
RANDOM_SHAPES = [(2, 1, 1, 0, 1), (2, 2, 1, 2, 2), (2, 3, 3, 2, 1), (2, 4, 1, 0, 3), (3, 1, 2, 1, 1), (3, 2, 1, 2, 1), (3, 3, 1, 0, 2),
                 (3, 4, 3, 1, 1), (4, 1, 1, 2, 3), (4, 2, 3, 0, 1), (4, 3, 2, 1, 1), (4, 4, 1, 1, 1), (2, 3, 1, 2, 1), (4, 2, 1, 0, 2)]
