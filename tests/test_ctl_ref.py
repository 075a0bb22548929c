"""tests/ctl_ref.py pinned: prove -> verify of the three-table system of tests/ctl_instances.py for both hashers, tampering rejected
(a ctl_zs_last word, a looked row, a filter bit), the generic CTL evaluator and the hand-written closures agreeing constraint by
constraint, the CTL Z order against a list written out by hand, the wire format through plonky2_gpu_amd.stark's parser, the Python
description validator on every refusal of gl_stark_tables_create, and Challenger::compact in both branches. Pure Python."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_instances as ci  # noqa: E402
import ctl_ref as cr  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import stark_ref as sr  # noqa: E402
from oracle import fri_ref  # noqa: E402
from plonky2_gpu_amd import stark as pstark  # noqa: E402
from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, StarkTablesDesc, TableWithColumns  # noqa: E402

P = sr.P
HASHERS = {"poseidon": gr.PoseidonHasher(), "keccak": gr.KeccakHasher()}
# hasher, num_challenges, declared constraint degree, rate_bits, cap_height. Keccak with two challenges and degree 3 would commit
# quotient leaves of 4 elements: degree 4 there (quotient_degree_factor 3, the trim of a factor that is no power of two)
CASES = [("poseidon", 2, 3, 1, 1), ("keccak", 1, 3, 1, 0), ("keccak", 2, 4, 2, 2), ("poseidon", 1, 3, 1, 3)]
_proofs = {}


def _case(i):
    """(system, num_challenges, fri_params, hasher, proofs): proved once, never changed (the tests copy what they tamper with)"""
    if i not in _proofs:
        hasher, nch, degree, rate_bits, cap_height = CASES[i]
        system = ci.system(degree)
        fp = ci.fri_params(rate_bits=rate_bits, cap_height=cap_height, arity_bits=ci.ARITY_BITS if cap_height < 2 else ((), (), ()))
        _proofs[i] = (system, nch, fp, HASHERS[hasher], cr.prove_tables(HASHERS[hasher], system, nch, fp, ci.make_traces(i)))
    return _proofs[i]


def test_the_traces_satisfy_every_constraint_and_every_lookup():
    system = ci.system()
    for seed in (0, 1, 2):
        assert ci.check_traces(system, ci.make_traces(seed))
    broken = ci.make_traces(0)
    broken[1][3][0] = (broken[1][3][0] + 1) % P
    assert not cr.product_identity_holds(system.lookups, broken, (5, 6))


@pytest.mark.parametrize("i", range(len(CASES)))
def test_prove_then_verify(i):
    system, nch, fp, hasher, proofs = _case(i)
    assert cr.verify_tables(hasher, system, nch, fp, proofs)
    assert cr.verify_tables(hasher, system, nch, fp, proofs, evaluator="closure")
    for k, proof in enumerate(proofs):
        assert len(proof["openings"]["ctl_zs_last"]) == len(ci.ZS_ORDER_2[k]) * nch // 2


def test_the_closure_evaluator_proves_the_same_bytes():
    system, nch, fp, hasher, proofs = _case(0)
    again = cr.prove_tables(hasher, system, nch, fp, ci.make_traces(0), evaluator="closure")
    assert cr.proofs_bytes(hasher, again) == cr.proofs_bytes(hasher, proofs)


def test_a_tampered_ctl_zs_last_word_is_rejected():
    system, nch, fp, hasher, proofs = _case(0)
    for k in range(3):
        bad = copy.deepcopy(proofs)
        bad[k]["openings"]["ctl_zs_last"][-1] = (bad[k]["openings"]["ctl_zs_last"][-1] + 1) % P
        with pytest.raises(AssertionError):
            cr.verify_tables(hasher, system, nch, fp, bad)


def _proof_of_broken_traces(change):
    system, nch, fp, hasher, _ = _case(0)
    traces = ci.make_traces(0)
    change(traces)
    with pytest.raises(AssertionError):
        cr.prove_tables(hasher, system, nch, fp, traces)  # the prover's own debug_assert
    return system, nch, fp, hasher, cr.prove_tables(hasher, system, nch, fp, traces, check=False)


def test_a_tampered_looked_row_is_rejected():
    """t0 of a row of table 1 that lookup 0 selects: no constraint of table 1 sees it, only the cross-table product does"""
    def change(traces):
        row = traces[1][2].index(0)
        traces[1][0][row] = (traces[1][0][row] + 1) % P

    system, nch, fp, hasher, proofs = _proof_of_broken_traces(change)
    with pytest.raises(AssertionError, match="cross-table lookup"):
        cr.verify_tables(hasher, system, nch, fp, proofs)


def test_a_tampered_filter_bit_is_rejected():
    """c3 of table 0 cleared on a row: still binary and disjoint from c2, so table 0's constraints hold; one looking row is missing"""
    def change(traces):
        traces[0][3][5] = 0

    system, nch, fp, hasher, proofs = _proof_of_broken_traces(change)
    with pytest.raises(AssertionError, match="cross-table lookup"):
        cr.verify_tables(hasher, system, nch, fp, proofs)


def test_a_non_binary_filter_is_refused_by_the_prover():
    system = ci.system()
    traces = ci.make_traces(0)
    traces[0][2][3] = 2
    with pytest.raises(AssertionError, match="Non-binary filter"):
        cr.ctl_z_polys(system.lookups, 1, 0, traces[0], [(3, 4)])
    traces[0][2][3] = P + 1  # 1 as a field element (then c2 c3 = 0 may fail: the Zs do not care)
    assert cr.ctl_z_polys(system.lookups, 1, 0, traces[0], [(3, 4)])


@pytest.mark.parametrize("F", [sr.Base, sr.Ext])
def test_the_generic_ctl_evaluator_and_the_closures_agree_on_random_rows(F):
    rng = np.random.default_rng(5)
    word = lambda: int(rng.integers(0, P, dtype=np.uint64))  # noqa: E731
    elem = (lambda: word()) if F is sr.Base else (lambda: (word(), word()))
    system = ci.system()
    for nch in (1, 2, 3):
        challenges = [(word(), word()) for _ in range(nch)]
        for k, stark in enumerate(system.tables):
            sets = [[(word(), word()) for _ in range(nch)] for _ in range(sr.quotient_degree_factor(stark))]
            nz = sr.num_zs(stark, nch) + len(cr.ctl_zs_order(system.lookups, nch, k))
            for _ in range(3):
                local, nxt = [elem() for _ in range(stark.num_columns)], [elem() for _ in range(stark.num_columns)]
                zs, zs_next = [elem() for _ in range(nz)], [elem() for _ in range(nz)]
                emitted = []
                for evaluator in ("program", "closure"):
                    consumer = sr.Consumer(F, [word() for _ in range(nch)], elem(), elem(), elem())
                    consumer.z_last, consumer.lagrange_first, consumer.lagrange_last = F.lift(3), F.lift(5), F.lift(7)
                    cr.eval_vanishing_poly(F, system, k, nch, local, nxt, zs, zs_next, sets, challenges, consumer, evaluator)
                    emitted.append([tuple(e) if isinstance(e, (tuple, list)) else e for e in consumer.emitted])
                assert emitted[0] == emitted[1] and len(emitted[0]) > 2 * (nz - sr.num_zs(stark, nch))


def test_the_ctl_z_order_matches_the_list_written_out_by_hand():
    system = ci.system()
    desc = system.desc(ci.DEGREE_BITS, 2, ci.fri_params())
    key = lambda zs: [(li, c, id(twc)) for li, c, twc in zs]  # noqa: E731
    for k in range(3):
        assert key(cr.ctl_zs_order(system.lookups, 2, k)) == key(ci.ZS_ORDER_2[k]) == key(desc.ctl_zs(k))
    assert [desc.num_ctl_zs(k) for k in range(3)] == [6, 6, 2] and [desc.num_zs(k) for k in range(3)] == [6, 6, 3]
    flat = desc.flatten()
    assert flat["lookup_bounds"].tolist() == [0, 3, 5, 7] and flat["twc_table"].tolist() == [0, 0, 1, 1, 2, 0, 1]
    assert flat["twc_filter"].tolist()[3:] == [pstark._lib.GL_CTL_NO_FILTER] * 4 and all(f < flat["column_constants"].size for f in flat["twc_filter"][:3])


@pytest.mark.parametrize("i", range(len(CASES)))
def test_the_wire_format_round_trips_through_the_products_parser(i):
    system, nch, fp, hasher, proofs = _case(i)
    name = CASES[i][0]
    data = cr.proofs_bytes(hasher, proofs)
    desc = system.desc(ci.DEGREE_BITS, nch, fp)
    parsed = pstark.tables_proof_from_bytes(data, desc, name)
    assert pstark.tables_proof_to_bytes(parsed, desc, name) == data
    assert cr.verify_tables(hasher, system, nch, fp, parsed)
    with pytest.raises(ValueError):
        pstark.tables_proof_from_bytes(data + b"\0", desc, name)
    with pytest.raises(EOFError):
        pstark.tables_proof_from_bytes(data[:-1], desc, name)


def _desc(nch=2, degree=3, rate_bits=1, cap_height=0, lookups=None, degree_bits=ci.DEGREE_BITS):
    d = ci.system(degree).desc(degree_bits, nch, ci.fri_params(rate_bits=rate_bits, cap_height=cap_height))
    if lookups is not None:
        d.lookups = lookups
    return d


def refusals():
    """name -> (description, hasher) of everything gl_stark_tables_create refuses about the shape; shared with tests/test_gpu_ctl.py"""
    out = {}

    def add(name, d, hasher="poseidon"):
        out[name] = (d, hasher)

    for key, value in (("rate_bits", 2), ("cap_height", 1), ("proof_of_work_bits", 5), ("num_query_rounds", 7)):
        d = _desc()
        d.tables[1].fri_params[key] = value
        add("tables differ in " + key, d)
    d = _desc()
    d.tables[2].num_challenges = 1
    add("tables differ in num_challenges", d)
    d = _desc()
    d.tables[0].fri_params["hiding"] = True
    add("hiding", d)
    d = _desc()
    d.tables[1].degree_bits = 0
    add("a single table's refusal: degree_bits 0", d)
    d = _desc()
    d.tables[0].fri_params["reduction_arity_bits"] = [3, 3]
    add("a single table's refusal: FRI arity", d)
    d = _desc()
    d.tables[2].pairs = [[(0, 5)]]
    add("a single table's refusal: pair column out of range", d)
    d = _desc()
    d.tables[1].num_public_inputs = 1
    add("public inputs", d)
    add("a table no lookup names", _desc(lookups=[ci.LOOKUPS[0], ci.LOOKUPS[2]]))
    add("no lookups", _desc(lookups=[]))
    looked = TableWithColumns(1, [CtlColumn.single(4)])
    add("table out of range", _desc(lookups=ci.LOOKUPS + [CrossTableLookup([TableWithColumns(3, [CtlColumn.single(0)])], looked)]))
    add("column out of range", _desc(lookups=ci.LOOKUPS + [CrossTableLookup([TableWithColumns(2, [CtlColumn.single(5)])], looked)]))
    add("filter's column out of range",
        _desc(lookups=ci.LOOKUPS + [CrossTableLookup([TableWithColumns(2, [CtlColumn.single(0)], CtlColumn.sum([1, 7]))], TableWithColumns(1, [CtlColumn.single(4)], CtlColumn.single(2)))]))
    lk = CrossTableLookup([TableWithColumns(0, [CtlColumn.single(0)])], TableWithColumns(1, [CtlColumn.single(4)]))
    lk.looked_table = TableWithColumns(1, [CtlColumn.single(4), CtlColumn.single(3)])
    add("unequal column counts", _desc(lookups=ci.LOOKUPS + [lk]))
    lk = CrossTableLookup([TableWithColumns(0, [CtlColumn.single(0)])], TableWithColumns(1, [CtlColumn.single(4)]))
    lk.looked_table = TableWithColumns(1, [CtlColumn.single(4)], CtlColumn.single(2))
    add("mixed filters", _desc(lookups=ci.LOOKUPS + [lk]))
    lk = CrossTableLookup([TableWithColumns(0, [CtlColumn.single(0)])], TableWithColumns(1, [CtlColumn.single(4)]))
    lk.looking_tables = []
    add("no looking table", _desc(lookups=ci.LOOKUPS + [lk]))
    add("constraint_degree 2 with a filtered CTL Z", _desc(degree=2))
    d = _desc()
    d.tables[2].constraint_degree = 1
    add("constraint_degree 1 with an unfiltered CTL Z", d)
    # Keccak: with one challenge tables 0 and 1 have 3 CTL Zs each; one more lookup between them makes 4
    add("keccak: a Zs oracle of 4 polynomials", _desc(nch=1, lookups=ci.LOOKUPS + [ci.LOOKUPS[2]]), "keccak")
    return out


REFUSALS = refusals()


def test_the_constructor_of_a_lookup_enforces_the_reference_s_rules():
    one, two = [CtlColumn.single(0)], [CtlColumn.single(0), CtlColumn.single(1)]
    with pytest.raises(ValueError):
        CrossTableLookup([TableWithColumns(0, one)], TableWithColumns(1, two))
    with pytest.raises(ValueError):
        CrossTableLookup([TableWithColumns(0, one, CtlColumn.single(2))], TableWithColumns(1, one))
    with pytest.raises(ValueError):
        CrossTableLookup([], TableWithColumns(1, one))


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_the_description_validator_refuses(name):
    d, hasher = REFUSALS[name]
    with pytest.raises(ValueError):
        d.validate(hasher)


def test_the_description_validator_accepts_the_system():
    _desc().validate()
    _desc(nch=1).validate("keccak")
    _desc(nch=2, degree=4, rate_bits=2).validate("keccak")
    with pytest.raises(ValueError):
        _desc(nch=2).validate("keccak")  # quotient leaves of 4, as for a single table


def test_ctl_columns():
    c = CtlColumn.linear_combination([(1, P + 2), (0, -1)], -3)
    assert c.terms == [(1, 2), (0, P - 1)] and c.constant == P - 3
    assert CtlColumn.le_bits([3, 1]).terms == [(3, 1), (1, 2)] and CtlColumn.sum([2, 2]).terms == [(2, 1), (2, 1)]
    assert CtlColumn.constant(9).terms == [] and CtlColumn.constant(9).constant == 9 and CtlColumn.single(4).terms == [(4, 1)]
    row = [5, 7, 11]
    assert cr.eval_column(sr.Base, c, row) == (2 * 7 - 5 - 3) % P
    assert cr.eval_column(sr.Ext, c, [(x, 1) for x in row]) == ((2 * 7 - 5 - 3) % P, 1)


def test_compact_in_both_branches():
    """with an empty input buffer compact only clears the output buffer (the next challenge duplexes again); with a non-empty one it
    duplexes first. The host Challenger's compact is checked in tests/test_gpu_ctl.py, where it can permute."""
    ch = fri_ref.Challenger()
    ch.observe_elements(range(1, 9))  # a full block: duplexed, the input buffer is empty, eight outputs wait
    assert not ch.input_buffer and len(ch.output_buffer) == 8
    twin = ch.clone()
    state = cr.compact(ch)
    assert state == twin.sponge_state and ch.output_buffer == [] and ch.input_buffer == []
    twin.duplexing()
    assert ch.get_challenge() == twin.get_challenge() != twin.sponge_state[0]
    ch = fri_ref.Challenger()
    ch.observe_elements(range(1, 12))  # three elements wait in the input buffer
    twin = ch.clone()
    assert len(ch.input_buffer) == 3
    state = cr.compact(ch)
    twin.duplexing()
    assert state == twin.sponge_state and ch.output_buffer == [] and ch.input_buffer == []
    twin.duplexing()
    assert ch.get_n_challenges(3) == twin.get_n_challenges(3)
