"""The fixed list of tests/gate_fuzz.py, checked on the CPU — what tests/test_gpu_gate_fuzz.py runs on the device:

* coverage(): the list reaches what it is there for (all twenty gate kinds, two parameter sets of every kind that has parameters,
  one to four selector groups and challenges, and every item of the raw programs' list), so that a changed generator fails here;
* the two CPU references agree on exactly the words the device will see: for every gate of every family-A case, the emitted program
  under the opcode executor (tests/gate_exec.py) gives oracle/gates_ref.constraints on every leaf the kernel reads;
* every program of both families is valid under a restatement of the header's rules (gate_fuzz.validate), and every rule has a mutant
  that restatement refuses; no emitter and no committed program uses an index the device would have to mask;
* the reference on raw words equals the reference on the reduced words, canonical.

The references are computed once per process (gate_fuzz.reference_quotient is memoised). Measured: the whole file takes 4 s on one
core of a build container, the 26 references together 2 s of it; tests/test_stark_ref.py takes 7 s there, tests/test_lookup_ref.py 9 s,
tests/test_ctl_ref.py 10 s."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gate_fuzz as gf  # noqa: E402
from gate_exec import execute  # noqa: E402
from oracle import gates_ref, pyref  # noqa: E402
from plonky2_gpu_amd import gate_program as gp  # noqa: E402

P = gf.P


def test_the_list_reaches_what_it_is_there_for():
    cov = gf.coverage()
    assert set(cov["parameters"]) == set(gf.KINDS) and len(gf.KINDS) == 20
    few = {k: v for k, v in cov["parameters"].items() if k in gf.KINDS_WITH_PARAMETERS and len(v) < 2}
    assert not few, ("kinds with fewer than two parameter sets", few)
    assert cov["groups"] == {1, 2, 3, 4} and cov["challenges"] == {1, 2, 3, 4} and cov["degree_bits"] == {2, 3, 4, 5}
    assert cov["poseidon_cases"] == [gf.POSEIDON_CASE]  # exactly one: 8.5 s of hiprtc
    qdfs = cov["quotient_degree_factors"]
    assert qdfs.count(4) >= 2 and any(q & (q - 1) for q in qdfs)  # qdb < rate_bits twice; one factor that is no power of two
    assert cov["partial_products"] and cov["duplicate_gates"] and cov["one_real_gate"] and cov["spare_wires"]
    assert cov["gates_per_case"][0] >= 2 and cov["gates_per_case"][-1] == 9
    assert 14 <= len(gf.A_CASES) <= 18 and 8 <= len(gf.B_CASES) <= 12


def test_the_raw_programs_reach_every_item_of_their_list():
    cov = gf.coverage()
    assert cov["ops"] == set(range(11))
    assert cov["high_registers"] == {60, 61, 62, 63} and cov["max_live"] >= 40
    assert cov["accumulators_open"] == 4 and cov["open_at_gate_end"]
    assert {0, 32, 63} <= cov["mulk_shifts"]
    assert cov["acc_single_max"] and cov["acc_many_terms_max"] and cov["acc_restart"]
    missing = [(op, pos, hex(v)) for v in gf.IMM_VALUES for op in (gp.ADD, gp.SUB, gp.MUL) for pos in (0, 1) if (op, pos, v) not in cov["imm_operands"]]
    assert not missing, ("constants that are never this operand of this operation", missing)
    assert {2, gf.P + 2, gf.M64} <= cov["imm_kept"]  # LOAD_IMMs with a reader that takes a register
    assert cov["fewer_emits"] and cov["max_constraints"] == 256 and cov["emits_256"]
    assert cov["program_lengths"][0] == 8 and cov["program_lengths"][-1] >= 600
    lengths = [len(p) for i in gf.FAMILY_B for p in gf.fuzz_case(i)["programs"]]
    assert all(8 <= n <= 800 for n in lengths) and all(1 <= len(gf.fuzz_case(i)["programs"]) <= 4 for i in gf.FAMILY_B)
    planted = cov["planted"]
    variants = {p["variant"] for p in planted if p["what"] == "pattern"}
    assert variants == set(gf.REWRITABLE + gf.NEAR_MISSES)
    whats = {p["what"] for p in planted}
    assert {"four_accumulators_open", "accumulator_left_open", "accumulator_starts_from_zero", "acc_bounds", "immediate_that_stays"} <= whats
    # the gate after the one that leaves an accumulator open starts with that accumulator
    left = [p for p in planted if p["what"] == "accumulator_left_open"]
    again = [p for p in planted if p["what"] == "accumulator_starts_from_zero"]
    assert left and [(p["case"], p["gate"] + 1, p["q"]) for p in left] == [(p["case"], p["gate"], p["q"]) for p in again]
    # one subexpression in two gates of a case; one term multiset in ACC orders that differ
    shared = [(p["case"], tuple(p["columns"])) for p in planted if p["what"] == "shared_subexpression"]
    assert any(shared.count(s) >= 2 for s in shared)
    sums = {}
    for p in planted:
        if p["what"] == "weighted_sum":
            sums.setdefault((p["case"], tuple(p["columns"])), set()).add((p["gate"], tuple(p["order"])))
    assert any(len({g for g, _ in v}) >= 2 and len({o for _, o in v}) >= 2 for v in sums.values())
    # the cases whose rewrites the GPU test counts hold rewritable and non-rewritable forms
    for j in gf.NEAR_MISS_CASES:
        case = gf.fuzz_case(gf.FAMILY_B[j])
        forms = [p["rewritable"] for p in case["planted"] if p["what"] == "pattern"]
        assert any(forms) and not all(forms) and gf.planted_rewrites(case) == sum(forms)
    assert gf.planted_rewrites(gf.fuzz_case(gf.FAMILY_B[1])) == 6
    # 7 ACCRs, 4 different sums: 2^31 x ones twice, the weighted sum in three orders
    sums = gf.fuzz_case(gf.FAMILY_B[gf.SUMS_CASE])
    assert sum(1 for p in sums["programs"] for ins in p if ins[0] == gp.ACCR) == 7 and gf.distinct_wire_sums(sums) == 4


def test_the_lifted_cases_are_short_and_hold_the_eight_upstream_kinds():
    kinds = {k for i in gf.LIFTED_A for k, _ in gf.fuzz_case(i)["gates"]}
    assert {"arithmetic_extension", "mul_extension", "reducing", "reducing_extension", "exponentiation", "poseidon_mds", "low_degree_interpolation",
            "high_degree_interpolation"} <= kinds
    assert len(gf.LIFTED_A) == 3 and len(gf.LIFTED_B) == 2
    assert all(sum(len(p) for p in gf.fuzz_case(i)["programs"]) <= 700 for i in gf.LIFTED_A + [gf.FAMILY_B[j] for j in gf.LIFTED_B])


@pytest.mark.parametrize("i", [i for i in gf.CASES if i not in gf.FAMILY_B])
def test_executor_and_oracle_gates_agree_on_the_leaves_of_the_case(i):
    case, inp = gf.fuzz_case(i), gf.fuzz_inputs(i)
    ng = len(case["groups"])
    bits, step = case["degree_bits"] + gf.RATE_BITS, 1 << (gf.RATE_BITS - case["qdb"])
    wires, cs = inp["wires"].tolist(), inp["cs"].tolist()
    rows = [pyref.reverse_bits(t * step, bits) for t in range(case["rows_read"])]
    if i == gf.POSEIDON_CASE:
        rows = rows[:8]  # 4 255 instructions per row
    for (kind, param), prog in zip(case["gates"], case["programs"]):
        assert sum(1 for ins in prog if ins[0] == gp.EMIT) == gates_ref.num_constraints(kind, param)
        for row in rows:
            got = [v % P for v in execute(prog, case["immediates"], ng, cs[row], wires[row], inp["pih"])]
            assert got == gates_ref.constraints(kind, param, cs[row][ng:], wires[row], inp["pih"], gates_ref.Base), (gf.describe(case), kind, param, row)


@pytest.mark.parametrize("i", gf.CASES)
def test_every_program_is_valid_and_the_leaf_lengths_cover_what_it_loads(i):
    case = gf.fuzz_case(i)
    gf.validate(case["programs"], case["immediates"], case["num_gate_constraints"])
    loads = lambda op: [ins[2] for p in case["programs"] for ins in p if ins[0] == op]  # noqa: E731
    assert max(loads(gp.LOAD_WIRE) + [0]) + 1 + gf.SPARE_WIRES <= case["wires_len"]
    assert max(loads(gp.LOAD_CONST) + [0]) + 1 + len(case["groups"]) <= case["num_constants"]
    inp = gf.fuzz_inputs(i)
    assert inp["wires"].shape == (case["n_ext"], case["wires_len"]) and inp["cs"].shape == (case["n_ext"], case["num_constants"] + gf.ROUTED)
    assert inp["zs"].shape == (case["n_ext"], case["num_challenges"] * (1 + case["num_prods"])) and 32 <= case["n_ext"] <= 256


def _mutants():
    """(name, programs, immediates, num_gate_constraints) that break one rule each"""
    L, A, R, E, K = gp.LOAD_WIRE, gp.ACC, gp.ACCR, gp.EMIT, gp.MULK
    w = (1 << 32) - 1
    return [
        ("a read before a write", [[(gp.ADD, 1, 0, 0), (E, 0, 1, 0)]], [], 1),
        ("an ACC weight of 2^32", [[(L, 0, 0, 0), (A, 0, 0, 0), (R, 1, 0, 0), (E, 0, 1, 0)]], [1 << 32], 1),
        ("3 then 2^32 - 1", [[(L, 0, 0, 0), (A, 0, 0, 0), (A, 0, 0, 1), (R, 1, 0, 0), (E, 0, 1, 0)]], [3, w], 1),
        ("an ACCR with no ACC", [[(L, 0, 0, 0), (R, 1, 0, 0), (E, 0, 1, 0)]], [], 1),
        ("more emits than num_gate_constraints", [[(L, 0, 0, 0), (E, 0, 0, 0), (E, 0, 0, 0)]], [], 1),
        ("an unknown opcode", [[(L, 0, 0, 0), (11, 1, 0, 0), (E, 0, 0, 0)]], [], 1),
        ("an immediate index out of range", [[(gp.LOAD_IMM, 0, 1, 0), (E, 0, 0, 0)]], [5], 1),
        ("a register index of 64", [[(L, 0, 0, 0), (L, 64, 0, 0), (E, 0, 0, 0)]], [], 1),
        ("a source register of 64", [[(L, 0, 0, 0), (gp.ADD, 1, 64, 0), (E, 0, 1, 0)]], [], 1),
        ("an accumulator index of 4", [[(L, 0, 0, 0), (A, 4, 0, 0), (R, 1, 0, 0), (E, 0, 1, 0)]], [1], 1),
        ("a MULK shift of 64", [[(L, 0, 0, 0), (K, 1, 0, 64), (E, 0, 1, 0)]], [], 1),
        ("a LOAD_PI index of 4", [[(gp.LOAD_PI, 0, 4, 0), (E, 0, 0, 0)]], [], 1),
    ]


MUTANTS = _mutants()
ACCEPTED = [
    ("2^31 alone", [[(gp.LOAD_WIRE, 0, 0, 0), (gp.ACC, 0, 0, 0), (gp.ACCR, 1, 0, 0), (gp.EMIT, 0, 1, 0)]], [1 << 31], 1),
    ("2^31 on two accumulators", [[(gp.LOAD_WIRE, 0, 0, 0), (gp.ACC, 0, 0, 0), (gp.ACC, 1, 0, 0), (gp.ACCR, 1, 0, 0), (gp.ACCR, 2, 1, 0), (gp.EMIT, 0, 1, 0),
                                   (gp.EMIT, 0, 2, 0)]], [1 << 31], 2),
]


@pytest.mark.parametrize("name,programs,imms,ngc", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_restated_rules_refuse_a_mutant_of_every_kind(name, programs, imms, ngc):
    with pytest.raises(ValueError):
        gf.validate(programs, imms, ngc)


def test_the_restated_rules_accept_the_largest_sums():
    for name, programs, imms, ngc in ACCEPTED:
        gf.validate(programs, imms, ngc)


def _masked_indices(prog):
    """the instructions of a program whose indices the device would have to mask"""
    bad = []
    for pc, (op, dst, a, b) in enumerate(prog):
        reads = [a, b] if op in (gp.ADD, gp.SUB, gp.MUL) else [a] if op in (gp.EMIT, gp.MULK, gp.ACC) else []
        if any(r >= 64 for r in reads) or (op not in (gp.EMIT, gp.ACC) and dst >= 64) or (op == gp.ACC and dst >= 4) or (op == gp.ACCR and a >= 4) \
                or (op == gp.MULK and b >= 64) or (op == gp.LOAD_PI and a >= 4):
            bad.append((pc, op, dst, a, b))
    return bad


def test_no_emitter_and_no_committed_program_uses_an_index_that_would_be_masked():
    """gate_programs_validate refuses register indices >= 64, accumulator indices >= 4, MULK shifts >= 64 and LOAD_PI indices >= 4, which
    the interpreter and the generator used to mask silently: nothing the project emits or ships relies on the masking. The compiled-in
    ed25519 table and the Keccak-f table's program do not pass that validator; they are read here all the same."""
    import re

    import test_gate_emit as tge
    from plonky2_gpu_amd import ed25519_circuit as ed

    for kind, param in sorted(set(tge.CASES) | set(gf.CATALOG) | set(ed.GATES), key=str):
        assert not _masked_indices(gp.build_gate(kind, param, gp.ImmediatePool())), (kind, param)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "plonky2_gpu_amd", "csrc", "ed25519_gate_program.inc")).read()
    start = text.index("ED25519_INSTRS[")
    words = [int(x) for x in re.findall(r"\d+", text[text.index("{", start):text.index("};", start)].split("\n", 1)[1])]
    quads = [tuple(words[k:k + 4]) for k in range(0, len(words), 4)]
    assert len(quads) == 21467 and not _masked_indices(quads)
    from plonky2_gpu_amd import keccak_table as kt
    from plonky2_gpu_amd import stark as pstark

    instrs = [tuple(int(x) for x in row) for row in np.asarray(kt.program()[0]).reshape(-1, 4)]
    assert len(instrs) > 1000 and pstark.LOAD_NEXT == 11 and pstark.EMIT_LAST_ROW == 14
    # the STARK opcodes: LOAD_NEXT writes dst, the three further EMITs read a; LOAD_PI indexes the public inputs themselves there
    assert not _masked_indices([ins for ins in instrs if ins[0] <= gp.ACCR and ins[0] != gp.LOAD_PI])
    assert all(ins[1] < 64 if ins[0] == pstark.LOAD_NEXT else ins[2] < 64 for ins in instrs if ins[0] > gp.ACCR)


@pytest.mark.parametrize("i", [2, 8, len(gf.A_CASES) + 2])
def test_the_reference_on_raw_words_is_the_reference_on_reduced_words(i):
    """six gates among them the Poseidon gate, and the raw program with every constant: leaves, k_is, challenges and hash reduced mod p
    first give the same canonical output"""
    case, inp = gf.fuzz_case(i), gf.fuzz_inputs(i)
    red = lambda v: (np.asarray(v, dtype=np.uint64) % np.uint64(P)) if isinstance(v, np.ndarray) else [int(x) % P for x in v]  # noqa: E731
    reduced = {k: red(v) for k, v in inp.items()}
    for col in range(len(case["groups"])):
        assert (reduced["cs"][:, col] % np.uint64(P) == reduced["cs"][:, col]).all()
    got = gf.reference_quotient(i)
    assert got.dtype == np.uint64 and got.shape == (case["num_challenges"], case["rows_read"]) and (got < np.uint64(P)).all()
    assert (inp["wires"] >= np.uint64(P)).any() and (gf.quotient_of(case, reduced) == got).all()
