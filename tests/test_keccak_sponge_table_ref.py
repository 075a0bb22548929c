"""The Keccak sponge table on the CPU: tests/keccak_sponge_table_ref.py (the reference's rows, its keccak_sponge_log and the
list of TODOs as constraints, restated from the Rust) against Keccak-256 and against its own constraints;
plonky2_gpu_amd/keccak_sponge_table.py (the constraints as a register program, the columns, the lookup descriptions) and the native
emitter gl_keccak_sponge_table_program against the restatement; the three derived lists against the lookups with tests/ctl_ref.py.
Everything is exact; nothing here needs a GPU."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref  # noqa: E402
import keccak_ref  # noqa: E402
import keccak_sponge_table_instances as ki  # noqa: E402
import keccak_sponge_table_ref as kr  # noqa: E402
import keccak_table_ref  # noqa: E402
import logic_table_ref  # noqa: E402
import memory_table_ref  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = kr.P
EMIT_KIND = {sr.EMIT: "plain", sr.EMIT_TRANSITION: "transition", sr.EMIT_FIRST_ROW: "first_row", sr.EMIT_LAST_ROW: "last_row"}


@functools.lru_cache(maxsize=None)
def _program():
    from plonky2_gpu_amd import keccak_sponge_table as ks

    return ks.program()


@functools.lru_cache(maxsize=None)
def _mixed_trace():
    """22 rows in 32: rows 0 .. 21 the twelve operations of ki.mixed(), ten padding rows"""
    cols = kr.trace_of_ops(ki.mixed())
    assert cols.shape == (414, 32)
    cols.setflags(write=False)
    return cols


def _digest(row):
    return b"".join(int(row[c]).to_bytes(4, "little") for c in kr.COL["updated_state_u32s"][:8])


# ---------------------------------------------------------------- the trace
def test_generation_vector_of_the_reference():
    """keccak_sponge_stark.rs test_generation: input [1, 2, 3] at (0, Segment::Code, 0), timestamp 0: one row whose first eight output
    limbs are Keccak-256 of the input"""
    rows = kr.generate_rows_for_op(kr.KeccakSpongeOp(0, kr.SEGMENT_CODE, 0, 0, bytes([1, 2, 3])))
    assert len(rows) == 1
    assert _digest(rows[-1]) == keccak_ref.keccak256(bytes([1, 2, 3]))
    assert _digest(rows[-1]).hex() == "f1885eda54b7a053318cd41e2093220dab15d65381b1157a3633a83bfd5c9239"  # the published value


@pytest.mark.parametrize("length", [0, 3, 135, 136, 137] + ki.LENGTHS[8:])
def test_last_row_holds_keccak_256_of_the_input(length):
    o = ki.op(length, 3)
    rows = kr.generate_rows_for_op(o)
    assert len(rows) == length // 136 + 1
    assert _digest(rows[-1]) == keccak_ref.keccak256(o.input)
    col = lambda name, i=0: kr.COL[name][i]  # noqa: E731
    for j, row in enumerate(rows):
        last = j == len(rows) - 1
        assert (row[col("is_full_input_block")], row[col("is_final_block")]) == ((0, 1) if last else (1, 0))
        assert [row[col(name)] for name in ("context", "segment", "virt", "timestamp", "len")] == [o.context, o.segment, o.virt, o.timestamp, length]
        assert row[col("already_absorbed_bytes")] == 136 * j
        remainder = length - 136 * j
        assert [row[c] for c in kr.COL["is_final_input_len"]] == [int(last and i == remainder) for i in range(136)]
        block = list(o.input[136 * j : 136 * (j + 1)])
        if last:
            block += [0x81] if remainder == 135 else [1] + [0] * (134 - remainder) + [0x80]
        assert [row[c] for c in kr.COL["block_bytes"]] == block and all(row[c] < 1 << 32 for c in range(414))
        before = [row[c] for c in kr.COL["original_rate_u32s"]]
        words = [int.from_bytes(bytes(block[4 * i : 4 * i + 4]), "little") for i in range(34)]
        assert [row[c] for c in kr.COL["xored_rate_u32s"]] == [a ^ b for a, b in zip(before, words)]
        if j:
            assert before + [row[c] for c in kr.COL["original_capacity_u32s"]] == [rows[j - 1][c] for c in kr.COL["updated_state_u32s"]]
        else:
            assert not any(before) and not any(row[c] for c in kr.COL["original_capacity_u32s"])


def test_rows_follow_the_list_and_padding_rows_are_zero():
    cols = _mixed_trace()
    assert kr.rows_needed(ki.mixed()) == 22 == sum(length // 136 + 1 for length in ki.LENGTHS)
    assert not cols[:, 22:].any()
    assert cols[kr.COL["context"][0], :22].tolist() == [k for k, length in enumerate(ki.LENGTHS) for _ in range(length // 136 + 1)]
    wide = kr.trace_of_ops(ki.mixed(), 6)
    assert wide.shape == (414, 64) and (wide[:, :32] == cols).all() and not wide[:, 32:].any()
    assert kr.trace_of_ops([]).shape == (414, 2) and not kr.trace_of_ops([]).any()
    with pytest.raises(AssertionError, match="cut an operation"):
        kr.trace_of_ops(ki.mixed(), 4)


def test_columns_are_the_reference_s():
    from plonky2_gpu_amd import keccak_sponge_table as ks

    starts = (ks.IS_FULL_INPUT_BLOCK, ks.IS_FINAL_BLOCK, ks.CONTEXT, ks.SEGMENT, ks.VIRT, ks.TIMESTAMP, ks.LEN, ks.ALREADY_ABSORBED_BYTES,
              ks.IS_FINAL_INPUT_LEN, ks.ORIGINAL_RATE_U32S, ks.ORIGINAL_CAPACITY_U32S, ks.BLOCK_BYTES, ks.XORED_RATE_U32S, ks.UPDATED_STATE_U32S)
    assert starts == (0, 1, 2, 3, 4, 5, 6, 7, 8, 144, 178, 194, 330, 364) == tuple(kr.COL[name].start for name, _ in kr.FIELDS)
    assert ks.NUM_COLUMNS == kr.NUM_COLUMNS == 414 and ks.OP_WORDS == kr.OP_WORDS == 5
    words, data = ks.ops_to_words([(o.context, o.segment, o.virt, o.timestamp, o.input) for o in ki.mixed()])
    ref_words, ref_data = kr.ops_to_words(ki.mixed())
    assert words.dtype == np.uint64 and data.dtype == np.uint8 and (words == ref_words).all() and (data == ref_data).all()
    assert ks.ops_to_words([])[0].shape == (0, 5) and ks.ops_to_words([])[1].size == 0


# ---------------------------------------------------------------- the program
def test_program_has_435_emits_of_the_stated_kinds_in_the_stated_order():
    from plonky2_gpu_amd import keccak_sponge_table as ks

    instrs, immediates = _program()
    sr.validate_program(instrs, immediates, ks.NUM_COLUMNS, 0)
    kinds = [EMIT_KIND[int(op)] for op in instrs[:, 0] if int(op) in EMIT_KIND]
    assert kinds == [kr.KINDS[name] for name, count in kr.GROUPS for _ in range(count)]
    assert len(kinds) == 435 == ks.NUM_CONSTRAINTS == kr.NUM_CONSTRAINTS
    assert [count for _, count in kr.GROUPS] == [3, 136, 1, 51, 51, 5, 50, 1, 1, 136]
    desc = ks.stark_desc(5, 2, si.fri_params(rate_bits=1))
    assert (desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.quotient_degree_factor) == (414, 0, 3, 2)
    assert desc.pairs == kr.KeccakSpongeTableStark.pairs == [] and desc.num_zs == 0


def test_native_emitter_gives_the_same_words():
    from plonky2_gpu_amd import keccak_sponge_table as ks

    instrs, immediates = _program()
    n_instrs, n_immediates, num_constraints = ks.native_program()
    assert n_instrs.shape == instrs.shape and (n_instrs == instrs).all()
    assert n_immediates == list(immediates) and num_constraints == 435


def test_program_and_closures_agree_on_random_rows():
    instrs, immediates = _program()
    rng = np.random.default_rng(414)
    for _ in range(6):
        local, nxt = ([int(v) % P for v in rng.integers(0, 1 << 64, size=kr.NUM_COLUMNS, dtype=np.uint64)] for _ in range(2))
        z_last, l_first, l_last = 5, 7, 11
        consumer = sr.Consumer(sr.Base, [3], z_last, l_first, l_last)
        sr.run_program(sr.Base, instrs, immediates, local, nxt, [], consumer)
        factor = {"plain": 1, "transition": z_last, "first_row": l_first}
        exp = [v * factor[kind] % P for kind, v in kr.eval_constraints(local, nxt)]
        assert len(consumer.emitted) == 435 and all(exp)
        assert consumer.emitted == exp
        by_closure = sr.Consumer(sr.Base, [3], z_last, l_first, l_last)
        kr.KeccakSpongeTableStark.closure(sr.Base, local, nxt, [], by_closure)
        assert by_closure.emitted == exp and by_closure.accs == consumer.accs


# ---------------------------------------------------------------- the constraints on the trace
def _program_violations(cols):
    """as kr.violations, through the register program: z_last = 0 on the last row, l_first = 1 on row 0 alone"""
    instrs, immediates = _program()
    n, bad = cols.shape[1], []
    for r in range(n):
        local, nxt = [int(v) for v in cols[:, r]], [int(v) for v in cols[:, (r + 1) % n]]
        consumer = sr.Consumer(sr.Base, [3], int(r != n - 1), int(r == 0), int(r == n - 1))
        sr.run_program(sr.Base, instrs, immediates, local, nxt, [], consumer)
        bad += [(r,) + kr.group_of(k) for k, v in enumerate(consumer.emitted) if v]
    return bad


@pytest.mark.parametrize("which", ["mixed", "empty", "full", "system"])
def test_an_honest_trace_satisfies_every_constraint_on_every_row(which):
    """"full": 8 rows and no padding row (the last row is a final row; nothing wraps); "empty": padding alone"""
    ops = {"mixed": ki.mixed, "empty": lambda: [], "full": lambda: [ki.op(length, k) for k, length in enumerate([300, 136, 0, 135, 5])],
           "system": ki.system_ops}[which]()
    cols = _mixed_trace() if which == "mixed" else kr.trace_of_ops(ops)
    assert which != "full" or (cols.shape == (414, 8) and cols[1, 7] == 1)
    assert kr.violations(cols) == [] == _program_violations(cols)


# rows of ki.mixed(): 0 .. 5 one final row each (lengths 0, 1, 3, 4, 134, 135), 6 .. 7 length 136 (full, final), 8 .. 9 length 137,
# 10 .. 11 length 271 (final remainder 135), 12 .. 14 length 272 (full, full, final), 15 .. 17, 18 .. 21, then ten padding rows.
# (column, row, change) -> the violations, worked out by hand from the list of constraints
TAMPER = {
    # L = 2 on a padding row: L (L - 1), sum d - L, and the dummy row before it sees a used row; (1 - F - L) next is (-1) 0 there
    "flags": ((1, 27, 2), [(26, "dummy_then_dummy", 0), (27, "flags", 1), (27, "final_len_sum", 0)]),
    "flags: both": ((0, 9, 1), None),
    "final_len_boolean": ((8 + 77, 26, 2), [(26, "final_len_boolean", 77), (26, "final_len_sum", 0), (26, "final_len_value", 77)]),
    # L = 1 on the last row, whose transitions do not count
    "final_len_sum": ((1, 31, 1), [(30, "dummy_then_dummy", 0), (31, "final_len_sum", 0)]),
    "first_row": ((178 + 3, 0, 9), [(0, "first_row", 34 + 3)]),
    # original_rate_u32s[2] of row 1, which follows the final row 0 and is a final row itself: nothing else reads it
    "after_final": ((144 + 2, 1, 9), [(0, "after_final", 2)]),
    "same_op": ((5, 12, "flip"), [(12, "same_op", 3)]),
    "state_carried": ((364 + 40, 8, "flip"), [(8, "state_carried", 40)]),
    # already_absorbed_bytes of the middle row of three: the constraint of the row before and its own
    "absorbed_carried": ((7, 13, "flip"), [(12, "absorbed_carried", 0), (13, "absorbed_carried", 0)]),
    # F = 1 on a padding row: the dummy row before it, and its own "plus 136"
    "dummy_then_dummy": ((0, 30, 1), [(29, "dummy_then_dummy", 0), (30, "absorbed_carried", 0)]),
    "final_len_value": ((6, 4, "flip"), [(4, "final_len_value", 134)]),
}


@pytest.mark.parametrize("what", sorted(TAMPER))
def test_one_changed_cell_breaks_the_family_it_should(what):
    """For each of the ten families a cell whose change makes that family fail — alone where a cell exists that no other family
    reads (first_row, after_final, same_op, state_carried, final_len_value), else with exactly the listed neighbours, which read the
    same cell.
    Through the closures and through the program: the same constraints, and only they, are non-zero."""
    (column, row, change), expected = TAMPER[what]
    cols = _mixed_trace().copy()
    cols[column, row] = cols[column, row] ^ np.uint64(1) if change == "flip" else change
    got = kr.violations(cols)
    assert got == _program_violations(cols)
    if expected is None:  # row 9 is a final row that also claims to be full: F L, and what F switches on towards row 10
        assert (9, "flags", 2) in got and {g[0] for g in got} == {9}
        assert {g[1] for g in got} == {"flags", "same_op", "state_carried", "absorbed_carried", "dummy_then_dummy"}
    else:
        assert sorted(got) == sorted(expected)
    assert what.split(":")[0] in {g[1] for g in got}


def test_every_family_has_a_tamper_case():
    assert {what.split(":")[0] for what in TAMPER} == {name for name, _ in kr.GROUPS}


# ---------------------------------------------------------------- the lookups
def test_lookup_descriptions_are_the_reference_s_words():
    from plonky2_gpu_amd import keccak_sponge_table as ks

    single = lambda c: [(c, 1)]  # noqa: E731
    assert [c.terms for c in ks.ctl_looked_data()] == [single(c) for c in (2, 3, 4, 6, 5)] + [single(364 + i) for i in range(8)]
    assert ks.ctl_looked_filter().terms == single(1)
    assert [c.terms for c in ks.ctl_looking_keccak()] == [single(c) for c in list(range(144, 194)) + list(range(364, 414))]
    assert [c.terms for c in ks.ctl_looking_keccak(xored=True)] == [single(c) for c in list(range(330, 364)) + list(range(178, 194)) + list(range(364, 414))]
    assert ks.ctl_looking_keccak_filter().terms == [(0, 1), (1, 1)] == ks.ctl_looking_logic_filter().terms
    for i in (0, 57, 135):
        m = ks.ctl_looking_memory(i)
        assert [(c.terms, c.constant) for c in m] == [([], 1), (single(2), 0), (single(3), 0), ([(4, 1), (7, 1)], i), (single(194 + i), 0)] + [([], 0)] * 7 + [(single(5), 0)]
        assert ks.ctl_looking_memory_filter(i).terms == [(0, 1)] + [(8 + k, 1) for k in range(i, 136)]
        assert ks.ctl_looking_memory_filter(i, strict=True).terms == [(0, 1)] + [(8 + k, 1) for k in range(i + 1, 136)]
    assert ks.num_logic_ctls() == 5
    for i in range(5):
        lg = ks.ctl_looking_logic(i)
        k = 8 if i < 4 else 2
        assert len(lg) == 27 and [(c.terms, c.constant) for c in lg[:3]] == [([], 0), ([], 0), ([], 1)]
        assert [c.terms for c in lg[3:11]] == [single(144 + 8 * i + j) for j in range(k)] + [[]] * (8 - k)
        assert [c.terms for c in lg[11:19]] == [[(194 + 32 * i + 4 * j + b, 1 << (8 * b)) for b in range(4)] for j in range(k)] + [[]] * (8 - k)
        assert [c.terms for c in lg[19:27]] == [single(330 + 8 * i + j) for j in range(k)] + [[]] * (8 - k)
        assert all(c.constant == 0 for c in lg[3:])


@functools.lru_cache(maxsize=None)
def _system_traces(lengths=ki.SYSTEM_LENGTHS):
    """the five traces of the system as lists of columns, from the reference models alone: the three lists are
    keccak_sponge_log's, computed from the inputs"""
    ops = ki.system_ops() if lengths == ki.SYSTEM_LENGTHS else [ki.op(length, k) for k, length in enumerate(lengths)]
    keccak_inputs, logic_ops, memory_ops = kr.log_of_ops(ops)
    rows = kr.rows_needed(ops)
    assert keccak_inputs.shape == (rows, 25) and logic_ops.shape == (5 * rows, 17) and memory_ops.shape == (sum(lengths), 14)
    as_lists = lambda cols: [[int(v) for v in col] for col in cols]  # noqa: E731
    sponge = as_lists(kr.trace_of_ops(ops, 3))
    keccak = as_lists(keccak_table_ref.generate_trace_rows(keccak_inputs, 128).T)
    logic = as_lists(logic_table_ref.trace_of_words(logic_ops, 5))
    memory = as_lists(memory_table_ref.trace_of_words(memory_ops)[0]) if len(memory_ops) >= 2 else None
    return [sponge, keccak, logic, memory, ki.cpu_trace(ops)]


CHALLENGE = (0x123456789ABCDEF, 0xFEDCBA987654321)


def test_the_derived_lists_fit_the_logic_memory_and_sponge_lookups():
    """at the system's sizes (sponge 8 rows, Keccak-f 128, logic 32, memory 512, the stand-in 4): what the sponge looks with is,
    as a multiset, what the looked table offers — with ctl_looking_logic_filter() and the strict memory filter; and with remainders
    4 and 28 the reference's own logic filter selects the same rows"""
    traces = _system_traces()
    assert [len(t[0]) for t in traces] == [8, 128, 32, 512, 4] and 24 * 5 <= 128 < 24 * 6
    assert ctl_ref.product_identity_holds(ki.lookups(("logic", "memory", "sponge")), traces, CHALLENGE)
    assert ctl_ref.product_identity_holds(ki.lookups(("logic",), logic_filter="reference"), traces, CHALLENGE)
    twcs = ki.lookups(("logic",))[0].looking_tables + ki.lookups(("logic",), logic_filter="reference")[0].looking_tables
    zs = [ctl_ref.partial_products(traces[ki.SPONGE], twc, CHALLENGE) for twc in twcs]
    assert zs[:5] == zs[5:]
    assert sum(len(lk.looking_tables) for lk in ki.lookups()) - 1 == 142  # on the sponge: 1 + 5 + 136 looking, and once looked


def test_the_keccak_lookup_holds_against_the_permutation_s_own_input_and_output():
    """What the sponge sends with xored=True is (input, output) of Keccak-f for every row that absorbs a block: checked against
    tests/keccak_ref.py directly and against the first and last row of each permutation of the Keccak-f table's trace."""
    traces = _system_traces()
    sponge, keccak = traces[ki.SPONGE], traces[ki.KECCAK]
    from plonky2_gpu_amd import keccak_sponge_table as ks

    for r in range(5):
        row = [col[r] for col in sponge]
        sent = [ctl_ref.eval_column(sr.Base, c, row) for c in ks.ctl_looking_keccak(xored=True)]
        lanes = [sent[2 * j] | sent[2 * j + 1] << 32 for j in range(25)]
        out = [int(x) for x in keccak_ref.keccak_f1600(np.array(lanes, dtype=np.uint64))]
        assert [sent[50 + 2 * j] | sent[50 + 2 * j + 1] << 32 for j in range(25)] == out
        first, last = [col[24 * r] for col in keccak], [col[24 * r + 23] for col in keccak]
        assert [first[keccak_table_ref.reg_input_limb(i)] for i in range(50)] == sent[:50]
        assert [last[keccak_table_ref.reg_output_limb(i)] for i in range(50)] == sent[50:]


# ---------------------------------------------------------------- the descriptions that cannot hold as written
def test_ctl_looking_keccak_as_written_sends_the_state_before_the_xor():
    """one block: original_rate_u32s is zero, Keccak-f received the padded block. The sponge's own rows show it: with xored=False the
    "input" half is not what the output half is the permutation of."""
    from plonky2_gpu_amd import keccak_sponge_table as ks

    cols = kr.trace_of_ops(ki.single(3))
    row = [int(v) for v in cols[:, 0]]
    for xored, holds in ((False, False), (True, True)):
        sent = [ctl_ref.eval_column(sr.Base, c, row) for c in ks.ctl_looking_keccak(xored=xored)]
        lanes = [sent[2 * j] | sent[2 * j + 1] << 32 for j in range(25)]
        out = [int(x) for x in keccak_ref.keccak_f1600(np.array(lanes, dtype=np.uint64))]
        assert ([sent[50 + 2 * j] | sent[50 + 2 * j + 1] << 32 for j in range(25)] == out) == holds


def test_the_keccak_f_table_s_own_lookup_offers_round_23_s_input():
    """Why ctl_keccak stays out of the accepted system even with xored=True: the Keccak-f table's ctl_data reads reg_a on the row
    its filter selects, the row of round 23 (keccak_stark.rs:34-43) — the state entering the last round, not the permutation's
    input (tests/test_gpu_keccak_table.py has the same finding). The products differ for either spelling of the looker."""
    traces = _system_traces()
    for xored in (False, True):
        assert not ctl_ref.product_identity_holds(ki.lookups(("keccak",), xored=xored), traces, CHALLENGE)


def test_the_reference_s_logic_filter_switches_off_xors_that_were_pushed():
    """a final remainder of 2 bytes: is_final_input_len[2] is not part of the sums from 3 or 4 on, so logic lookups 3 and 4 are off
    on that row, and the 5 XORs generation pushed for it are looked at by 3"""
    lengths = (2, 300)
    ops = [ki.op(length, k) for k, length in enumerate(lengths)]
    _, logic_ops, _ = kr.log_of_ops(ops)
    sponge = [[int(v) for v in col] for col in kr.trace_of_ops(ops, 3)]
    logic = [[int(v) for v in col] for col in logic_table_ref.trace_of_words(logic_ops, 5)]
    traces = [sponge, None, logic, None, None]
    assert ctl_ref.product_identity_holds(ki.lookups(("logic",)), traces, CHALLENGE)
    assert not ctl_ref.product_identity_holds(ki.lookups(("logic",), logic_filter="reference"), traces, CHALLENGE)
    selected = [sum(ctl_ref.eval_column(sr.Base, twc.filter_column, [col[0] for col in sponge]) for twc in lk.looking_tables)
                for lk in (ki.lookups(("logic",))[0], ki.lookups(("logic",), logic_filter="reference")[0])]
    assert selected == [5, 3]


def test_the_reference_s_memory_filter_reads_the_first_padding_byte():
    """is_final_input_len[i..] includes a remainder of exactly i bytes: lookup i is on although byte i is the padding's 0x01, which
    memory never saw. Every final row has such an i, so the lookup as written holds for no input; from i + 1 on it does."""
    traces = _system_traces()
    assert ctl_ref.product_identity_holds(ki.lookups(("memory",)), traces, CHALLENGE)
    assert not ctl_ref.product_identity_holds(ki.lookups(("memory",), memory_strict=False), traces, CHALLENGE)
    row = [col[1] for col in traces[ki.SPONGE]]  # the final row of the 140-byte operation: remainder 4
    on = [i for i in range(136) if ctl_ref.eval_column(sr.Base, ki.lookups(("memory",), memory_strict=False)[0].looking_tables[i].filter_column, row)]
    assert on == [0, 1, 2, 3, 4] and row[kr.COL["block_bytes"][4]] == 1


# ---------------------------------------------------------------- one whole proof
def test_the_reference_prover_proves_the_table_and_its_verifier_accepts():
    """8 rows (the system's sponge), rate 2, 2 challenges: stark_ref proves the program and verifies with the program and with the
    closures"""
    import generic_prove_ref as gr
    from oracle import accel

    instrs, immediates = _program()
    stark = kr.KeccakSpongeTableStark(instrs, immediates)
    fp = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,))
    hasher = gr.PoseidonHasher()
    with accel.c_backend():
        proof = sr.prove(hasher, stark, 2, fp, _system_traces()[ki.SPONGE], [])
        assert sr.verify(hasher, stark, 2, fp, proof)
        assert sr.verify(hasher, stark, 2, fp, proof, evaluator="closure")
    assert len(proof["openings"]["local_values"]) == 414 and len(proof["openings"]["quotient_polys"]) == 4
