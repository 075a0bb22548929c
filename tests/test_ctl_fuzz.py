"""tests/ctl_fuzz.py pinned on the CPU: what its fixed list of multi-table systems reaches — a CONDITION on the generator and its
seeds, asserted here, not a measurement —, that every system is valid (the description validator, every constraint on every row,
the product identity of every lookup), that tests/ctl_ref.py proves and verifies it, that its lookups bind (a cell only a lookup
reads, changed: the verifier's cross-table product fails) and the order of the CTL Zs of a table that looks into itself. The
reference runs with oracle.accel.c_backend (its hashes, trees and transforms in C); the algebra of the STARKs stays Python."""
import copy
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_fuzz as cf  # noqa: E402
import ctl_ref as cr  # noqa: E402
import stark_ref as sr  # noqa: E402
from oracle import accel  # noqa: E402
from test_ctl_ref import HASHERS  # noqa: E402

P = sr.P
ALL = range(len(cf.CASES))


def test_the_fixed_list_reaches_what_the_generator_is_for():
    every = list(ALL)
    assert 12 <= len(every) <= 16
    assert cf.coverage() == {
        "table_counts": {"poseidon": [2, 3, 8, 16], "keccak": [2, 9, 17]},
        "num_challenges": {"poseidon": [1, 2, 3, 4], "keccak": [1, 2, 3, 4]},
        "columns_of_8_plus_tables": [3, 4, 5],
        "degree_bits_of_8_plus_tables": [1, 2, 3],
        "degree_bits": [1, 2, 3, 4, 5, 11, 12],
        "two_rows_beside_2_11": [11],
        "rows_2_12": [12],
        "pair_two_ctl_zs_qdf_3": [4, 5, 14],
        "qdf_4_rate_bits_2": [0, 2, 3, 6, 7, 8, 9, 13, 14],
        "qdf_rate_bits": [(2, 1), (2, 2), (3, 2), (4, 2)],
        "self_lookup": [1, 2],
        "repeated_looking": [0, 1, 6],
        "mixed_roles": [0, 1, 2, 3, 5, 7, 8, 9, 10],
        # Poseidon: 4 is the last leaf that is not hashed, 5 the first that is, 8 / 9 the sponge's rate and one more; Keccak: the
        # neighbours of the refused 4
        "zs_widths": {"poseidon": [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 36], "keccak": [1, 2, 3, 5, 6, 8]},
        "widths": [1, 2, 3, 4, 5],
        "looking_twcs": [1, 2, 3],
        "general_side": {"poseidon": ["looked", "looking"], "keccak": ["looked", "looking"]},
        "column_kinds": ["combination", "combination+constant", "constant", "le_bits", "single"],
        "filter_kinds": ["not", "single", "sum"],
        "filter_selects_no_row": [0, 1, 2, 3, 5, 6, 7, 8, 9, 10],
        "filter_selects_every_row": [1, 4, 6, 7, 9, 10, 11, 12],
        "unfiltered_with_default": [0, 9, 13],
        "unfiltered_without_default": [1, 5, 7, 8, 9, 10, 13, 14],
        "only_looking_or_only_looked": [1, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14],
        "cap_is_the_smallest_lde": [7, 11],
        "arity_lists_differ_one_empty": [0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13],
        "proof_of_work": [0, 1, 2, 3, 5, 7, 9, 10, 11, 12, 13, 14],
    }


def test_the_generator_is_deterministic():
    a = cf.fuzz_system(3)
    b = cf._draw_system(cf.np.random.default_rng(cf.seed_of(3)), cf.CASES[3])
    assert a.traces == b.traces and a.fri_params == b.fri_params and a.filters == b.filters
    fa, fb = a.desc().flatten(), b.desc().flatten()
    assert sorted(fa) == sorted(fb) and all((fa[k] == fb[k]).all() for k in fa)
    assert all((s.instrs == t.instrs).all() and s.immediates == t.immediates for s, t in zip(a.system.tables, b.system.tables))


@pytest.mark.parametrize("i", ALL)
def test_every_system_is_valid_and_its_traces_satisfy_it(i):
    case = cf.fuzz_system(i)
    assert case.system.ctl_closures is None
    case.desc().validate(case.hasher)
    for stark in case.system.tables:
        sr.validate_program(stark.instrs, stark.immediates, stark.num_columns, 0)
        assert stark.constraint_degree in (3, 4, 5)
    assert cf.check_traces(case)
    # what the description says a filter selects is what it selects
    for (li, j), (_, count, n) in case.filters.items():
        twc = case.system.lookups[li].twcs[j]
        trace = case.traces[twc.table]
        values = [cr.eval_column(cr.Base, twc.filter_column, [col[r] for col in trace]) for r in range(n)]
        assert len(trace[0]) == n and sorted(values) == [0] * (n - count) + [1] * count


@functools.lru_cache(maxsize=None)
def reference(i):
    """(case, proofs) of case i: proved once, never changed; shared with tests/test_gpu_ctl_fuzz.py"""
    case = cf.fuzz_system(i)
    with accel.c_backend():
        return case, cr.prove_tables(HASHERS[case.hasher], case.system, case.num_challenges, case.fri_params, case.traces)


@pytest.mark.parametrize("i", ALL)
def test_prove_then_verify(i):
    case, proofs = reference(i)
    with accel.c_backend():
        assert cr.verify_tables(HASHERS[case.hasher], case.system, case.num_challenges, case.fri_params, proofs)
    for k, proof in enumerate(proofs):
        assert len(proof["openings"]["permutation_ctl_zs"]) == cf.zs_widths(case)[k]


def lookup_only_cell(case):
    """(table, column, row) of the first cell that a CTL column reads with a non-zero coefficient on a row its TWC's filter selects
    and that neither the table's program nor a permutation pair reads; None if there is none"""
    for lk in case.system.lookups:
        for twc in lk.twcs:
            stark, trace = case.system.tables[twc.table], case.traces[twc.table]
            taken = {int(r[2]) for r in stark.instrs if int(r[0]) in (sr.LOAD_WIRE, sr.LOAD_NEXT)} | {c for pair in stark.pairs for cp in pair for c in cp}
            for row in range(len(trace[0])):
                values = [col[row] for col in trace]
                if twc.filter_column is not None and cr.eval_column(cr.Base, twc.filter_column, values) != 1:
                    continue
                for col in twc.columns:
                    for c, k in col.terms:
                        if k and c not in taken:
                            return twc.table, c, row
    return None


@pytest.mark.parametrize("i", ALL)
def test_the_lookups_bind(i):
    """every table's own constraints still hold (the changed column is no constraint's), every FRI proof is good: only the
    cross-table product can refuse"""
    case = cf.fuzz_system(i)
    hasher = HASHERS[case.hasher]
    cell = lookup_only_cell(case)
    assert cell is not None, "no cell that only a lookup reads on a row it selects"
    table, column, row = cell
    traces = copy.deepcopy(case.traces)
    traces[table][column][row] = (traces[table][column][row] + 1) % P
    assert not cr.product_identity_holds(case.system.lookups, traces, (5, 6))
    with accel.c_backend():
        proofs = cr.prove_tables(hasher, case.system, case.num_challenges, case.fri_params, traces, check=False)
        with pytest.raises(AssertionError, match="cross-table lookup"):
            cr.verify_tables(hasher, case.system, case.num_challenges, case.fri_params, proofs)


def test_the_ctl_zs_of_a_table_that_looks_into_itself_are_ordered_by_hand():
    """case 2, four challenges: table 2 is the second looking table and the looked table of lookup 1. Per challenge the looking TWCs
    in list order, then the looked TWC (cross_table_lookup_data, cross_table_lookup.rs:245-309)"""
    case = cf.fuzz_system(2)
    assert case.num_challenges == 4 and len(case.system.lookups) == 2
    lk = case.system.lookups[1]
    assert [t.table for t in lk.looking_tables] == [1, 2] and lk.looked_table.table == 2
    looking, looked = lk.looking_tables[1], lk.looked_table
    assert looking is not looked
    by_hand = [(1, 0, looking), (1, 0, looked), (1, 1, looking), (1, 1, looked), (1, 2, looking), (1, 2, looked), (1, 3, looking), (1, 3, looked)]
    key = lambda zs: [(li, c, id(twc)) for li, c, twc in zs]  # noqa: E731
    assert key(cr.ctl_zs_order(case.system.lookups, 4, 2)) == key(by_hand) == key(case.desc().ctl_zs(2))
    flat = case.desc().flatten()
    assert flat["lookup_bounds"].tolist() == [0, 2, 5] and flat["twc_table"].tolist() == [0, 1, 1, 2, 2]
