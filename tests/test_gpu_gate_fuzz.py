"""The gate kernels of gl_compute_quotient_polys on the fixed list of tests/gate_fuzz.py — random gate lists of all twenty kinds and raw
register programs that go where the emitters do not, on ANY u64 words — bit for bit against references that share no code with the
device: there is no tolerance anywhere, every comparison is equality of u64 words.

Every case runs on four routes: the interpreter (csrc/plonk.hip, eval_gate_program) and the kernel csrc/gate_jit.hip generates, each
on leaf-major leaves and on column-major leaves (guarded and padded, at the smallest legal pitch and at that + 6). What the list reaches
is asserted on the CPU (tests/test_gate_fuzz.py); here, besides the outputs: what the generator made of the list (units, biases,
rewritten range checks), the column_stride rule, the limit of 256 constraints, the validator, the indices it no longer masks, and the
generator's variants (the diagnostic library's switches, one child process per setting).

Every compilation goes to a kernel cache in a temporary directory: the code under test is what the current generator emits, and the
shipped cache is untouched. The hiprtc time of every case is printed (pytest -s); DESIGN.md 6 has the figures measured on the GPU
host."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gate_fuzz as gf  # noqa: E402
import gate_fuzz_device as gd  # noqa: E402
import gate_fuzz_variant_child as child  # noqa: E402
import test_gate_fuzz as tgf  # noqa: E402  (MUTANTS, ACCEPTED: the programs the restated rules refuse and accept)
from gpu_util import gpu, kernel_cache  # noqa: E402,F401

P = gf.P
LIFTED = gf.LIFTED_A + [gf.FAMILY_B[j] for j in gf.LIFTED_B]
GENERATED = {}  # case -> gd.generated(...) of the product library's kernel, filled as the cases run


def _check_case(gpu, i, lifted=False):
    case, inp = gf.fuzz_case(i), gf.fuzz_inputs(i)
    exp = gf.reference_quotient(i)
    what = dict(gf.describe(case), lifted=False)
    if lifted:
        inp, what["lifted"] = gd.lifted_inputs(inp, seed=i)
        assert what["lifted"] > 0
    prog = gd.program(gpu, case, inp)
    seconds = gd.compile_program(prog, case)
    GENERATED[i] = gd.generated(prog)
    print("case %d (%s, %d instructions): gl_gate_kernel_build %.1f s, %s" % (i, case["family"], sum(len(p) for p in case["programs"]), seconds, GENERATED[i]))
    routes = gd.run_routes(gpu, case, inp, prog)
    assert len(routes) == 6  # interpreter and compiled x leaf-major and two column pitches
    for route, got in routes:
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (route, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad), what)
        assert (got < np.uint64(P)).all(), (route, "an output word is not canonical", what)


@pytest.mark.gpu
@pytest.mark.parametrize("i", gf.CASES)
def test_quotient_of_a_fuzz_case_on_all_four_routes(gpu, i):
    _check_case(gpu, i)


@pytest.mark.gpu
@pytest.mark.parametrize("i", LIFTED)
def test_quotient_with_every_liftable_word_lifted_by_p(gpu, i):
    """leaves, k_is, challenges and hash as x + p wherever that fits 64 bits: the output is that of the unlifted inputs"""
    _check_case(gpu, i, lifted=True)


def _generated(gpu, i):
    if i not in GENERATED:  # run on its own: compile now (into the module's cache)
        case, inp = gf.fuzz_case(i), gf.fuzz_inputs(i)
        prog = gd.program(gpu, case, inp)
        gd.compile_program(prog, case)
        GENERATED[i] = gd.generated(prog)
    return GENERATED[i]


@pytest.mark.gpu
def test_what_the_generator_did_with_the_list(gpu):
    """counts the generator of the fuzz cases knows, read off gl_gate_kernel_source; no source is pinned"""
    made = {i: _generated(gpu, i) for i in gf.CASES if i != gf.POSEIDON_CASE or i in GENERATED}
    assert any(len(m["gates_per_unit"]) == 1 and m["gates_per_unit"][0] >= 2 for m in made.values()), "no case is one unit of several gates"
    assert any(len(m["gates_per_unit"]) >= 2 for m in made.values()), "no case is cut into several units"
    assert any(m["bias"] for m in made.values()), "no case carries a bias"
    assert any(made[i]["rewrites"] > 0 and made[i]["bias"] for i in gf.FAMILY_B), "no raw program has the range-check pattern rewritten"
    # one accumulator per different sum: the same terms in another ACC order, in another gate, are the same value
    sums = gf.fuzz_case(gf.FAMILY_B[gf.SUMS_CASE])
    assert made[sums["index"]]["sums"] == gf.distinct_wire_sums(sums), (gf.describe(sums), made[sums["index"]])
    for j in gf.NEAR_MISS_CASES:  # the bias is applied exactly when the rewrite is: the outputs of these cases are checked above
        i = gf.FAMILY_B[j]
        assert made[i]["rewrites"] == gf.planted_rewrites(gf.fuzz_case(i)), (gf.describe(gf.fuzz_case(i)), made[i])


def _refused(call):
    import plonky2_gpu_amd as pg

    with pytest.raises(pg.Plonky2HipError) as e:
        call()
    assert e.value.code == pg.GL_E_INVALID and str(e.value).strip(), (e.value.code, str(e.value))
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("compiled", [False, True], ids=["interpreter", "compiled"])
def test_a_column_stride_below_the_rows_read_is_refused_and_nothing_is_written(gpu, compiled):
    import plonky2_gpu_amd as pg

    i = 2  # quotient degree 4: the kernel reads 64 of the 128 leaves
    case, inp = gf.fuzz_case(i), gf.fuzz_inputs(i)
    assert case["rows_read"] < case["n_ext"]
    prog = gd.program(gpu, case, inp)
    if compiled:
        gd.compile_program(prog, case)
    lay = gd.ColumnMajor(gpu, case, inp, case["rows_read"])
    marker = np.full(case["num_challenges"] * case["rows_read"], gd.MARKER, dtype=np.uint64)
    out = pg.DeviceBuffer.from_host(gpu, marker)
    try:
        _refused(lambda: gd.quotient(gpu, case, inp, lay.ptrs, prog, compiled, case["rows_read"] - 1, out=out))
        assert (out.download() == marker).all()
        lay.check_unchanged()
        got = gd.quotient(gpu, case, inp, lay.ptrs, prog, compiled, case["rows_read"], out=out)  # the same buffers at the legal pitch
        assert (got == gf.reference_quotient(i)).all()
    finally:
        out.free()
        lay.free()


@pytest.mark.gpu
def test_257_constraints_are_refused_by_the_interpreter_route_and_nothing_is_written(gpu):
    """256 (GP_MAX_CONSTRAINTS) passes on all routes: case LIMIT_CASE of the list above"""
    import plonky2_gpu_amd as pg

    i = gf.FAMILY_B[gf.LIMIT_CASE]
    case, inp = gf.fuzz_case(i), gf.fuzz_inputs(i)
    assert case["num_gate_constraints"] == 256
    prog = gd.program(gpu, case, inp)
    lay = gd.LeafMajor(gpu, inp)
    marker = np.full(case["num_challenges"] * case["rows_read"], gd.MARKER, dtype=np.uint64)
    out = pg.DeviceBuffer.from_host(gpu, marker)
    try:
        _refused(lambda: gd.quotient(gpu, case, inp, lay.ptrs, prog, False, out=out, num_gate_constraints=257))
        assert (out.download() == marker).all()
        lay.check_unchanged()
        _refused(lambda: prog.compile(257, case["num_challenges"]))
    finally:
        out.free()
        lay.free()


def _raw_program(gpu, programs, imms):
    import plonky2_gpu_amd as pg

    return pg.GateProgram(gpu, programs, [0] * len(programs), [(0, len(programs))], [0, 0, 0, 0], immediates=imms or None)


REFUSED_BY_BUILD = {"a read before a write": "read before any write", "an ACC weight of 2^32": "2^32", "3 then 2^32 - 1": "2^63",
                    "an ACCR with no ACC": "nothing was added", "more emits than num_gate_constraints": "num_gate_constraints",
                    "an unknown opcode": "unknown opcode", "an immediate index out of range": "out of range",
                    "a register index of 64": "register index >= 64", "a source register of 64": "register index >= 64",
                    "an accumulator index of 4": "accumulator index >= 4", "a MULK shift of 64": "MULK shift >= 64",
                    "a LOAD_PI index of 4": "LOAD_PI index >= 4"}
INDEX_MUTANTS = [m for m in tgf.MUTANTS if ">= " in REFUSED_BY_BUILD[m[0]]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,programs,imms,ngc", tgf.MUTANTS, ids=[m[0] for m in tgf.MUTANTS])
def test_gate_kernel_build_refuses_what_the_rules_refuse(gpu, name, programs, imms, ngc):
    """with a message that names the rule; nothing is compiled or launched"""
    prog = _raw_program(gpu, programs, imms)
    message = _refused(lambda: prog.compile(ngc, 2))
    assert REFUSED_BY_BUILD[name] in message, message
    assert not prog.kernel


@pytest.mark.gpu
@pytest.mark.parametrize("name,programs,imms,ngc", tgf.ACCEPTED, ids=[m[0] for m in tgf.ACCEPTED])
def test_gate_kernel_build_accepts_the_largest_sums(gpu, name, programs, imms, ngc):
    prog = _raw_program(gpu, programs, imms)
    prog.compile(ngc, 2)
    assert prog.kernel


def _create_interpreted_circuit(gpu, programs, imms):
    """gl_circuit_create with compile_gates = 0 — the route on which the interpreter's programs are validated — for the tiny circuit of
    tests/plonk_instance.py with ITS gate programs replaced by `programs` (one selector group)"""
    from plonk_instance import make_circuit

    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib, gate_program as gp

    circuit = make_circuit(4, seed=1)[0]
    instrs, descs = gp.pack_program(programs, [0] * len(programs), [(0, len(programs))])
    instrs, descs = np.ascontiguousarray(instrs), np.ascontiguousarray(descs)
    im = np.array(imms, dtype=np.uint64) if imms else None
    fp = circuit["fri_params"]
    arity = np.ascontiguousarray(fp["reduction_arity_bits"], dtype=np.uint32)
    u64 = lambda v: np.ascontiguousarray(np.array(v, dtype=np.uint64))  # noqa: E731
    k_is, consts, sigmas = u64(circuit["k_is"]), u64(circuit["constants"]), u64(circuit["sigmas"])
    desc = _lib.GlCircuitDesc(
        ctypes.sizeof(_lib.GlCircuitDesc), circuit["degree_bits"], circuit["num_wires"], circuit["num_routed_wires"], circuit["num_constants"],
        circuit["num_challenges"], circuit["quotient_degree_factor"], circuit["num_gate_constraints"],
        _lib.GlFriParams(fp["rate_bits"], fp["cap_height"], fp["proof_of_work_bits"], fp["num_query_rounds"], arity.size, arity.ctypes.data, 0),
        k_is.ctypes.data, consts.ctypes.data, sigmas.ctypes.data, instrs.ctypes.data, instrs.size // 4, descs.ctypes.data, descs.size // 6,
        im.ctypes.data if im is not None else None, 0 if im is None else im.size, 1, 0, None)
    h = ctypes.c_void_p()
    _lib.call("gl_circuit_create_h", _lib.GL_HASHER_POSEIDON, ctypes.byref(desc), ctypes.byref(h), gpu.ptr)
    _lib.load().gl_circuit_destroy(h.value)
    assert pg is not None


@pytest.mark.gpu
def test_indices_that_used_to_be_masked_are_refused_on_both_routes(gpu):
    """register indices >= 64, accumulator indices >= 4, MULK shifts >= 64 and LOAD_PI indices >= 4: gate_programs_validate refuses
    them for the compiled kernel (test_gate_kernel_build_refuses_what_the_rules_refuse) and, here, for the circuit whose gates the
    interpreter runs. The same circuit with a program that keeps the rules is created."""
    name, programs, imms, ngc = tgf.ACCEPTED[0]
    _create_interpreted_circuit(gpu, programs, imms)
    assert len(INDEX_MUTANTS) == 5
    for name, programs, imms, ngc in INDEX_MUTANTS:
        message = _refused(lambda: _create_interpreted_circuit(gpu, programs, imms))
        assert REFUSED_BY_BUILD[name] in message, (name, message)


VARIANTS = [{"PLONKY2_HIP_JIT_FUSE_GATES": "1"}, {"PLONKY2_HIP_JIT_FUSE": "0"}, {"PLONKY2_HIP_JIT_FUSE": "0", "PLONKY2_HIP_JIT_PEEPHOLE": "0"},
            {"PLONKY2_HIP_JIT_PREFETCH": "0"}]


@pytest.fixture(scope="module")
def product_digests(gpu, kernel_cache):
    """sha256 of the product library's compiled outputs of the LIFTED cases (they equal the references: asserted here too)"""
    out = {}
    for i in LIFTED:
        outputs, _ = child.compiled_outputs(gpu, i)
        assert all((got == gf.reference_quotient(i)).all() for _, got in outputs)
        out[i] = child.digest(outputs)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("env", VARIANTS, ids=[" ".join("%s=%s" % kv for kv in v.items()).replace("PLONKY2_HIP_JIT_", "") for v in VARIANTS])
def test_generator_variants_give_the_product_library_s_outputs(gpu, product_digests, kernel_cache, env):
    """one fresh child process per setting (the diagnostic library reads the switches), one child alive at a time"""
    debug_lib = os.path.join(ROOT, "plonky2_gpu_amd", "libplonky2_hip_debug.so")
    assert os.path.exists(debug_lib), "make -C plonky2_gpu_amd/csrc debug (done by __graft_entry__.build())"
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PLONKY2_HIP_JIT_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gate_fuzz_variant_child.py")] + [str(i) for i in LIFTED],
                       env=dict(clean, PLONKY2_HIP_LIBRARY=debug_lib, PLONKY2_HIP_KERNEL_CACHE=kernel_cache, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    print(r.stdout)
    for i in LIFTED:
        assert "sha256 %d %s " % (i, product_digests[i]) in r.stdout, (env, gf.describe(gf.fuzz_case(i)), r.stdout[-800:])
    if env.get("PLONKY2_HIP_JIT_PEEPHOLE") == "0":  # the switch was read: nothing is rewritten
        assert all(line.endswith("rewrites 0") for line in r.stdout.splitlines() if line.startswith("sha256 "))


def test_the_digest_is_of_the_output_words():
    a = np.arange(6, dtype=np.uint64).reshape(2, 3)
    assert child.digest([("x", a)]) == hashlib.sha256(a.tobytes()).hexdigest()
