"""Random multi-table STARK systems with cross-table lookups that are valid by construction (TEST INFRASTRUCTURE ONLY).

fuzz_system(i) builds entry i of the fixed list CASES: a tests/ctl_instances.py System without hand-written closures (the "program"
evaluator of tests/ctl_ref.py runs it), the tables' degree_bits, num_challenges, one FRI dict per table, the hasher's name and
traces that satisfy every constraint and every lookup. An entry of CASES fixes what the list exists to reach (the hasher, the
heights, the number of challenges, which table looks into which); everything else — widths, which side of a lookup is the general
one, coefficients, filters, how many rows a filter selects, the rows, the FRI shape where the entry leaves it open — is drawn from
np.random.default_rng(seed_of(i)), so a case never changes.

A table: column 0 counts from START (a first-row and a transition constraint); optionally column 1 is the degree-3 recurrence of
tests/ctl_instances.py, x' = x^2 c0 + K; every flag column f has f (f - 1) = 0 and two flags of one filter f g = 0; optionally one
permutation pair (a free column, a shuffled copy of it). The program reads no other column: those belong to the lookups.

A lookup: one side (the looked table, or every looking table) has general CtlColumns over its table's free columns — single
columns, combinations with any coefficient in [0, p) and a non-zero constant, constant-only columns, le_bits — and its tuples are
what tests/ctl_ref.py's eval_column gives; the other side has CtlColumn.single over columns of its own, which receive those tuples in
shuffled order on the rows its filter selects and random words elsewhere. Filters are single(flag), 1 - flag or the sum of two
disjoint flags, and select 0 .. n rows. Lookups without filters have equal total heights, or taller looking sides and a default
tuple on the surplus rows.

KeccakHash<25> cannot hash a leaf of 4 elements: where the trace, the Zs oracle or the quotient oracle of a table would be 4 wide
under Keccak the generator draws again (the free columns, the constraint degree, at last the whole system); no case is skipped.

coverage() is what tests/test_ctl_fuzz.py pins, so that a change of the generator that loses a path fails on the CPU."""
import functools

import numpy as np

import ctl_instances as ci
import ctl_ref as cr
import representatives as rep
import stark_ref as sr
from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, StarkAsm, TableWithColumns

P = ci.P
START, K = ci.START, ci.K
SEED = 41000

# What an entry may fix: hasher, nch, degree_bits (per table); lookups [(looked, (looking, ..), kind)] with kind "filtered" /
# "plain" (no filters, no default, equal heights) / "default" / None (drawn among what the heights allow), or chain=True: a random
# chain through all tables, every table with 3 - 5 columns; degree / pairs / recur per table; rate_bits, cap_height, arity (per
# table), pow, rounds; counts {(lookup, twc): rows its filter selects}; max_width. What is absent is drawn.
CASES = [
    # 0: three tables, all drawn
    dict(hasher="poseidon", nch=2, degree_bits=(3, 3, 2), lookups=[(1, (0, 0), None), (2, (1,), None), (0, (2, 1), None)]),
    # 1: Keccak Zs oracles of 3 and of 5; a table twice in one lookup; a table looking into itself
    dict(hasher="keccak", nch=1, degree_bits=(3, 4), pairs=(), lookups=[(1, (0, 0), "filtered"), (1, (0, 1), "filtered"), (1, (1,), None)]),
    # 2: four challenges under Poseidon: Zs oracles of 4 (the last leaf that is not hashed), 8 and 9; table 2 looks into itself and has
    # quotient_degree_factor 4 at rate_bits 2
    dict(hasher="poseidon", nch=4, degree_bits=(2, 3, 3), degree=(3, 4, 5), pairs=(2,), rate_bits=2, lookups=[(1, (0,), None), (2, (1, 2), "filtered")]),
    # 3: four challenges under Keccak
    dict(hasher="keccak", nch=4, degree_bits=(4, 3), pairs=(), lookups=[(1, (0,), "filtered"), (0, (1,), None)]),
    # 4: a pair, 3 CTL Zs and quotient_degree_factor 3 together; a Zs oracle of 3
    dict(hasher="poseidon", nch=3, degree_bits=(5, 4), degree=(3, 4), pairs=(1,), lookups=[(1, (0,), "filtered")]),
    # 5: a Zs oracle of 5: one permutation Z and four CTL Zs
    dict(hasher="poseidon", nch=2, degree_bits=(4, 4), degree=(4, 3), pairs=(0,), lookups=[(1, (0,), "plain"), (0, (1,), "filtered")]),
    # 6: a Zs oracle of 36
    dict(hasher="poseidon", nch=4, degree_bits=(3, 3), pairs=(), max_width=2, lookups=[(1, (0, 0, 0), "filtered")] * 3),
    # 7 - 10: eight tables (one step of the trace caps, `last` at once), nine (a second step of one cap), sixteen (two full steps),
    # seventeen (three)
    dict(hasher="poseidon", nch=2, chain=8),
    dict(hasher="keccak", nch=3, chain=9, filtered_tables=(8,)),
    dict(hasher="poseidon", nch=1, chain=16),
    dict(hasher="keccak", nch=1, chain=17),
    # 11: 2 rows beside 2^11 (two scan blocks); the cap is the small table's whole LDE; arity lists that differ, one of them empty
    dict(hasher="poseidon", nch=1, degree_bits=(1, 11), degree=(3, 3), pairs=(), recur=(False, True), rate_bits=1, cap_height=2, arity=((), (3, 2)),
         pow=3, rounds=2, max_width=2, lookups=[(1, (0,), "filtered")], counts={(0, 0): 2}),
    # 12: 2^12 rows (four scan blocks) under Keccak
    dict(hasher="keccak", nch=1, degree_bits=(12, 5), degree=(3, 3), pairs=(), recur=(False, False), rate_bits=1, rounds=2, max_width=2,
         lookups=[(0, (1,), "filtered")], counts={(0, 0): 32}),
    # 13: no filters: a default and unequal heights, and equal heights without a default
    dict(hasher="poseidon", nch=3, degree_bits=(3, 2, 3), lookups=[(1, (0,), "default"), (2, (0,), "plain")]),
    # 14: Keccak with two challenges: no quotient_degree_factor 2, a Zs oracle of 3 from one permutation Z and two CTL Zs
    dict(hasher="keccak", nch=2, degree_bits=(4, 4), degree=(4, 5), pairs=(0,), lookups=[(1, (0,), "plain")]),
]


def seed_of(i):
    return SEED + i


class Case:
    """what fuzz_system returns; `filters` {(lookup, twc index in lookup.twcs): (kind, rows selected)}, `general` per lookup"""

    def __init__(self, system, degree_bits, num_challenges, fri_params, hasher, traces, filters, general):
        self.system, self.degree_bits, self.num_challenges, self.fri_params = system, degree_bits, num_challenges, fri_params
        self.hasher, self.traces, self.filters, self.general = hasher, traces, filters, general

    def desc(self, degree_bits=None):
        return self.system.desc(self.degree_bits if degree_bits is None else degree_bits, self.num_challenges, self.fri_params)


def _word(rng):
    return int(rng.integers(0, P, dtype=np.uint64))


class _Table:
    def __init__(self, rng, degree_bits):
        self.n = 1 << degree_bits
        self.cols = [[START + r for r in range(self.n)]]
        self.free, self.flags, self.disjoint, self.pairs, self.recur = [], [], [], [], None
        self.rng = rng

    def add(self, values):
        self.cols.append([int(v) for v in values])
        return len(self.cols) - 1

    def add_free(self):
        """mostly small words (they have a second representative word + p), some of the edges, the rest uniform"""
        self.free.append(self.add(rep.field_data(self.rng, self.n, small=0.4, edges=0.1)))

    def add_recurrence(self):
        x = [_word(self.rng)]
        for r in range(self.n - 1):
            x.append((x[r] * x[r] % P * self.cols[0][r] + K) % P)
        self.recur = self.add(x)

    def add_pair(self):
        src = self.free[int(self.rng.integers(0, len(self.free)))]
        self.pairs.append([(src, self.add([self.cols[src][k] for k in self.rng.permutation(self.n)]))])

    def add_filter(self, count, kinds):
        """(filter column, kind, the rows it selects in random order): `count` rows through flag columns of its own"""
        rng, n = self.rng, self.n
        rows = [int(r) for r in rng.permutation(n)[:count]]
        kind = kinds[int(rng.integers(0, len(kinds)))]
        flag = lambda on: self.add([1 if r in on else 0 for r in range(n)])  # noqa: E731
        if kind == "single":
            f = flag(set(rows))
            self.flags.append(f)
            return CtlColumn.single(f), kind, rows
        if kind == "not":
            f = flag(set(range(n)) - set(rows))
            self.flags.append(f)
            return CtlColumn.linear_combination([(f, P - 1)], 1), kind, rows
        cut = int(rng.integers(0, count + 1))
        f, g = flag(set(rows[:cut])), flag(set(rows[cut:]))
        self.flags += [f, g]
        self.disjoint.append((f, g))
        return CtlColumn.sum([f, g]), kind, rows

    def general_column(self):
        rng = self.rng
        pick = lambda: self.free[int(rng.integers(0, len(self.free)))]  # noqa: E731
        kind = int(rng.integers(0, 5))
        if kind == 0:
            return CtlColumn.single(pick())
        if kind == 1:
            return CtlColumn.constant(_word(rng))
        if kind == 2:
            return CtlColumn.le_bits([pick() for _ in range(int(rng.integers(1, 4)))])
        terms = [(pick(), _word(rng)) for _ in range(int(rng.integers(1, 4)))]
        return CtlColumn.linear_combination(terms, 1 + int(rng.integers(0, P - 1, dtype=np.uint64)) if kind == 3 else 0)

    def program(self):
        a = StarkAsm()
        c0 = a.local(0)
        a.emit_first_row(a.sub(c0, a.imm(START)))
        a.emit_transition(a.sub(a.next(0), a.add(c0, a.imm(1))))
        if self.recur is not None:
            x = a.local(self.recur)
            a.emit_transition(a.sub(a.sub(a.next(self.recur), a.mul(a.mul(x, x), c0)), a.imm(K)))
        for f in self.flags:
            x = a.local(f)
            a.emit(a.mul(x, a.sub(x, a.imm(1))))
        for f, g in self.disjoint:
            a.emit(a.mul(a.local(f), a.local(g)))
        return a


def _tuples(table, columns, rows):
    return [tuple(cr.eval_column(cr.Base, c, [col[r] for col in table.cols]) for c in columns) for r in rows]


def _draw_count(rng, n, room):
    u = rng.random()
    return min(room, 0 if u < 0.2 else n if u < 0.45 else int(rng.integers(0, n + 1)))


def _add_lookup(rng, tables, li, looked, looking, kind, general, width, counts, filter_kinds, filters):
    """appends the columns the lookup needs to its tables and returns the CrossTableLookup"""
    tl, tk = tables[looked], [tables[t] for t in looking]
    total = sum(t.n for t in tk)
    if kind is None:
        kinds = ["filtered"] + (["plain"] if total == tl.n else []) + (["default"] if total > tl.n and general == "looked" else [])
        kind = kinds[int(rng.integers(0, len(kinds)))]
    assert kind == "filtered" or (kind == "plain" and total == tl.n) or (kind == "default" and total > tl.n and general == "looked"), (li, kind)
    if kind == "filtered":
        room, sel = tl.n, []
        for j, t in enumerate(tk):
            sel.append(min(room, counts[(li, j)]) if (li, j) in counts else _draw_count(rng, t.n, room))
            room -= sel[-1]
    else:
        sel = [t.n for t in tk]
    twcs, rows = [None] * (len(tk) + 1), [None] * (len(tk) + 1)
    flt = [None] * (len(tk) + 1)

    def open_twc(j, t, count):
        if kind == "filtered":
            flt[j], fk, rows[j] = t.add_filter(count, filter_kinds)
            filters[(li, j)] = (fk, count, t.n)
        else:
            rows[j] = [int(r) for r in rng.permutation(t.n)]

    def single_side(j, t, index, tuples):
        own = [t.add([_word(rng) for _ in range(t.n)]) for _ in range(width)]
        for r, tup in zip(rows[j], tuples):
            for c, v in zip(own, tup):
                t.cols[c][r] = v
        twcs[j] = TableWithColumns(index, [CtlColumn.single(c) for c in own], flt[j])

    default = None
    if general == "looked":
        open_twc(len(tk), tl, sum(sel))
        columns = [tl.general_column() for _ in range(width)]
        twcs[-1] = TableWithColumns(looked, columns, flt[-1])
        pool = _tuples(tl, columns, rows[-1])
        if kind == "default":
            default = [_word(rng) for _ in range(width)]
            pool += [tuple(default)] * (total - tl.n)
        pool = [pool[k] for k in rng.permutation(len(pool))]
        for j, (t, index) in enumerate(zip(tk, looking)):
            open_twc(j, t, sel[j])
            single_side(j, t, index, pool[: sel[j]])
            pool = pool[sel[j] :]
        assert not pool
    else:
        pool = []
        for j, (t, index) in enumerate(zip(tk, looking)):
            open_twc(j, t, sel[j])
            columns = [t.general_column() for _ in range(width)]
            twcs[j] = TableWithColumns(index, columns, flt[j])
            pool += _tuples(t, columns, rows[j])
        pool = [pool[k] for k in rng.permutation(len(pool))]
        open_twc(len(tk), tl, len(pool))
        single_side(len(tk), tl, looked, pool)
    return CrossTableLookup(twcs[:-1], twcs[-1], default=default), kind


def _log2_ceil(x):
    return (x - 1).bit_length()


def _draw_system(rng, spec):
    keccak, nch = spec["hasher"] == "keccak", spec["nch"]
    chain = spec.get("chain")
    if chain:
        degree_bits = [int(rng.integers(1, 4)) for _ in range(chain)]
        order = [int(k) for k in rng.permutation(chain)]
        topology = [(order[k], (order[k + 1],), None) for k in range(chain - 1)]
        side = ["looked", "looking"][int(rng.integers(0, 2))]  # one side for the whole chain: no table pays for two single sides
        for k, (looked, looking, _) in enumerate(topology):
            if set((looked,) + looking) & set(spec.get("filtered_tables", ())):
                topology[k] = (looked, looking, "filtered")
    else:
        degree_bits, topology = list(spec["degree_bits"]), spec["lookups"]
    nt = len(degree_bits)
    tables = [_Table(rng, db) for db in degree_bits]
    recur = spec.get("recur", [False] * nt if chain else [bool(rng.integers(0, 2)) for _ in range(nt)])
    for t, r in zip(tables, recur):
        if r:
            t.add_recurrence()
        for _ in range(1 if chain else int(rng.integers(1, 4))):
            t.add_free()
    pairs = spec.get("pairs", () if chain else [k for k in range(nt) if rng.random() < 0.4])
    for k in pairs:
        tables[k].add_pair()
    lookups, filters, general, kinds = [], {}, [], []
    for li, (looked, looking, kind) in enumerate(topology):
        side_li = side if chain else "looked" if kind == "default" else ["looked", "looking"][int(rng.integers(0, 2))]
        width = 1 if chain else int(rng.integers(1, spec.get("max_width", 5) + 1))
        lk, kind = _add_lookup(rng, tables, li, looked, looking, kind, side_li, width, spec.get("counts", {}),
                               ("single", "not") if chain else ("single", "not", "sum"), filters)
        lookups.append(lk)
        general.append(side_li)
        kinds.append(kind)
    for t in tables:  # a chain's tables have 3 - 5 columns; no trace of 4 columns under Keccak
        while (chain and len(t.cols) < 3) or (keccak and len(t.cols) == 4):
            t.add_free()
        assert not chain or 3 <= len(t.cols) <= 5, len(t.cols)
    degree = list(spec.get("degree", [None] * nt))
    for k in range(nt):
        while degree[k] is None or (keccak and nch * (degree[k] - 1) == 4):
            degree[k] = int(rng.integers(3, 6))
    rate_bits = spec.get("rate_bits", max(_log2_ceil(d - 1) for d in degree))
    lde_bits = [db + rate_bits for db in degree_bits]
    cap_height = spec.get("cap_height", int(rng.integers(0, min(min(lde_bits), 3) + 1)))
    arity = spec.get("arity")
    if arity is None:
        arity = []
        for db in degree_bits:
            room, ab = min(db, db + rate_bits - cap_height), []
            while room >= (2 if keccak else 1) and rng.random() < 0.7:
                ab.append(int(rng.integers(2 if keccak else 1, min(room, 3) + 1)))
                room -= ab[-1]
            arity.append(ab)
    fri = ci.fri_params(rate_bits=rate_bits, cap_height=cap_height, arity_bits=arity, num_query_rounds=spec.get("rounds", int(rng.integers(1, 4))),
                        proof_of_work_bits=spec.get("pow", int(rng.integers(0, 4))))
    starks = [ci.Table("t%d" % k, len(t.cols), degree[k], t.pairs, t.program(), None) for k, t in enumerate(tables)]
    system = ci.System(starks, lookups, None)
    case = Case(system, degree_bits, nch, fri, spec["hasher"], [t.cols for t in tables], filters, general)
    case.kinds = kinds
    return case


def zs_widths(case):
    """per table: permutation Zs + CTL Zs"""
    nch = case.num_challenges
    return [sr.num_zs(t, nch) + len(cr.ctl_zs_order(case.system.lookups, nch, k)) for k, t in enumerate(case.system.tables)]


@functools.lru_cache(maxsize=None)
def fuzz_system(i):
    rng = np.random.default_rng(seed_of(i))
    for _ in range(100):
        case = _draw_system(rng, CASES[i])
        if case.hasher != "keccak" or 4 not in zs_widths(case):
            return case
    raise AssertionError("case %d: no system without a Keccak leaf of 4 in 100 draws" % i)


def check_traces(case, challenges=((0x1234567, 0x89ABCDEF), (P - 2, 1 << 40))):
    """every constraint of every table's program on every row, and the product identity of every lookup under two challenges"""
    for k, (stark, trace) in enumerate(zip(case.system.tables, case.traces)):
        n = len(trace[0])
        assert n == 1 << case.degree_bits[k] and len(trace) == stark.num_columns and all(len(c) == n and all(0 <= v < P for v in c) for c in trace)
        for r in range(n):
            local, nxt = [col[r] for col in trace], [col[(r + 1) % n] for col in trace]
            consumer = sr.Consumer(sr.Base, [1], 0 if r == n - 1 else 1, 1 if r == 0 else 0, 1 if r == n - 1 else 0)
            sr.eval_constraints(sr.Base, stark, local, nxt, [], consumer, "program")
            assert consumer.emitted and all(e == 0 for e in consumer.emitted), (k, "row", r, consumer.emitted)
        for pair in stark.pairs:
            for a, b in pair:
                assert sorted(trace[a]) == sorted(trace[b]), (k, pair)
    for c in challenges:
        assert cr.product_identity_holds(case.system.lookups, case.traces, c)
    return True


def coverage():
    """what CASES reaches, as plain data"""
    cases = [fuzz_system(i) for i in range(len(CASES))]
    by_hasher = lambda f: {h: sorted({x for c in cases if c.hasher == h for x in f(c)}) for h in ("poseidon", "keccak")}  # noqa: E731
    where = lambda f: [i for i, c in enumerate(cases) if f(c)]  # noqa: E731
    qdf = lambda c, k: sr.quotient_degree_factor(c.system.tables[k])  # noqa: E731
    rate = lambda c: c.fri_params[0]["rate_bits"]  # noqa: E731
    tables = lambda c: range(len(c.system.tables))  # noqa: E731
    nctl = lambda c, k: len(cr.ctl_zs_order(c.system.lookups, c.num_challenges, k))  # noqa: E731
    looking = lambda c: {t.table for lk in c.system.lookups for t in lk.looking_tables}  # noqa: E731
    looked = lambda c: {lk.looked_table.table for lk in c.system.lookups}  # noqa: E731
    column_kinds = set()
    for c in cases:
        for lk in c.system.lookups:
            for t in lk.twcs:
                for col in t.columns:
                    coeffs = [k for _, k in col.terms]
                    column_kinds.add("constant" if not coeffs else "single" if coeffs == [1] and not col.constant else
                                     "le_bits" if coeffs == [1 << j for j in range(len(coeffs))] and not col.constant else
                                     "combination+constant" if col.constant else "combination")
    return dict(
        table_counts=by_hasher(lambda c: [len(c.system.tables)]),
        num_challenges=by_hasher(lambda c: [c.num_challenges]),
        columns_of_8_plus_tables=sorted({t.num_columns for c in cases if len(c.system.tables) >= 8 for t in c.system.tables}),
        degree_bits_of_8_plus_tables=sorted({db for c in cases if len(c.system.tables) >= 8 for db in c.degree_bits}),
        degree_bits=sorted({db for c in cases for db in c.degree_bits}),
        two_rows_beside_2_11=where(lambda c: 1 in c.degree_bits and 11 in c.degree_bits),
        rows_2_12=where(lambda c: 12 in c.degree_bits),
        pair_two_ctl_zs_qdf_3=where(lambda c: any(c.system.tables[k].pairs and nctl(c, k) >= 2 and qdf(c, k) == 3 for k in tables(c))),
        qdf_4_rate_bits_2=where(lambda c: rate(c) == 2 and any(qdf(c, k) == 4 for k in tables(c))),
        qdf_rate_bits=sorted({(qdf(c, k), rate(c)) for c in cases for k in tables(c)}),
        self_lookup=where(lambda c: any(lk.looked_table.table in [t.table for t in lk.looking_tables] for lk in c.system.lookups)),
        repeated_looking=where(lambda c: any(len({t.table for t in lk.looking_tables}) < len(lk.looking_tables) for lk in c.system.lookups)),
        mixed_roles=where(lambda c: any(any(k in [t.table for t in a.looking_tables] and k == b.looked_table.table
                                            for a in c.system.lookups for b in c.system.lookups if a is not b) for k in tables(c))),
        zs_widths=by_hasher(zs_widths),
        widths=sorted({len(lk.looked_table.columns) for c in cases for lk in c.system.lookups}),
        looking_twcs=sorted({len(lk.looking_tables) for c in cases for lk in c.system.lookups}),
        general_side=by_hasher(lambda c: c.general),
        column_kinds=sorted(column_kinds),
        filter_kinds=sorted({v[0] for c in cases for v in c.filters.values()}),
        filter_selects_no_row=where(lambda c: any(count == 0 for _, count, n in c.filters.values())),
        filter_selects_every_row=where(lambda c: any(count == n for _, count, n in c.filters.values())),
        unfiltered_with_default=where(lambda c: "default" in c.kinds),
        unfiltered_without_default=where(lambda c: "plain" in c.kinds),
        only_looking_or_only_looked=where(lambda c: looking(c) ^ looked(c)),
        cap_is_the_smallest_lde=where(lambda c: c.fri_params[0]["cap_height"] == min(c.degree_bits) + rate(c)),
        arity_lists_differ_one_empty=where(lambda c: [] in [fp["reduction_arity_bits"] for fp in c.fri_params]
                                           and any(fp["reduction_arity_bits"] for fp in c.fri_params)),
        proof_of_work=where(lambda c: c.fri_params[0]["proof_of_work_bits"] > 0),
    )
