"""A long STARK program cut into unit programs (gl_stark_split_program, csrc/stark_split.hip) and the unit kernels compiled
without a device (gl_stark_precompile_units): nothing here needs a GPU, everything is exact.

1. the splitter's properties on the Keccak-f table's program (47 227 instructions), the memory table's, every description of
   tests/stark_fuzz.py and two hand-made programs: the units' EMIT runs partition the EMITs in order, tests/stark_ref.py's
   validate_program accepts every unit, no unit exceeds the cap unless it holds exactly one constraint, and a cap at or above the
   program's length gives the input word for word;
2. its semantics: on a few random rows of any u64 words the units, run in order by tests/stark_ref.py's interpreter, emit what
   the program emits — values and kinds;
3. the device-free compile in ONE child process with temporary kernel caches, as tests/test_stark_compile_cpu.py does it."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import representatives as rep  # noqa: E402
import stark_fuzz as sf  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = sr.P
KINDS = {sr.EMIT: "constraint", sr.EMIT_TRANSITION: "transition", sr.EMIT_FIRST_ROW: "first_row", sr.EMIT_LAST_ROW: "last_row"}


# ---------------------------------------------------------------- the programs
def _shared_first_value():
    """the first instruction's value is read by every one of 12 constraints: each unit has to compute it again"""
    instrs = [(sr.LOAD_WIRE, 7, 0, 0)]
    for k in range(12):
        instrs += [(sr.LOAD_NEXT, 1, k % 3, 0), (sr.MUL, 2, 1, 7), (sr.ADD, 2, 2, 7), ((sr.EMIT, sr.EMIT_TRANSITION)[k % 2], 0, 2, 0)]
    return np.array(instrs, dtype=np.uint16), [], 3, 0


def _acc_chain_across_a_cut():
    """accumulator 1 is summed over three ACCs with a constraint (and so a possible cut) behind each of the first two, while
    accumulator 0 is summed and read in between: the unit of the last constraint needs all three ACCs and none of accumulator 0"""
    imms = [3, 1 << 20, 5]
    instrs = [(sr.LOAD_WIRE, 0, 0, 0), (sr.LOAD_WIRE, 1, 1, 0), (sr.ACC, 1, 0, 0), (sr.EMIT, 0, 0, 0),
              (sr.LOAD_NEXT, 2, 2, 0), (sr.ACC, 1, 2, 1), (sr.ACC, 0, 1, 2), (sr.ACCR, 3, 0, 0), (sr.EMIT_FIRST_ROW, 0, 3, 0),
              (sr.ACC, 0, 2, 0), (sr.MUL, 4, 1, 2), (sr.ACC, 1, 4, 2), (sr.ACCR, 5, 1, 0), (sr.ACCR, 6, 0, 0), (sr.SUB, 5, 5, 6),
              (sr.EMIT_LAST_ROW, 0, 5, 0), (sr.LOAD_IMM, 9, 1, 0), (sr.EMIT, 0, 1, 0)]
    return np.array(instrs, dtype=np.uint16), imms, 3, 0


@functools.lru_cache(maxsize=None)
def _program(name):
    """(instrs, immediates, num_columns, num_public_inputs)"""
    if name == "keccak":
        from plonky2_gpu_amd import keccak_table as kt

        instrs, imms, _ = kt.native_program()
        return instrs, imms, kt.NUM_COLUMNS, 0
    if name == "memory":
        from plonky2_gpu_amd import memory_table as mt

        instrs, imms, _ = mt.native_program()
        return instrs, imms, mt.NUM_COLUMNS, 0
    if name == "shared":
        return _shared_first_value()
    if name == "acc":
        return _acc_chain_across_a_cut()
    s = sf.fuzz_case(int(name))["stark"]
    return s.instrs, s.immediates, s.num_columns, s.num_public_inputs


def _caps(name):
    n = len(_program(name)[0])
    if name == "keccak":
        return [250, 1500, 10 ** 6]
    if name == "memory":
        return [1, 40, n]
    if name in ("shared", "acc"):
        return [1, 3, 6, 9, n - 1, n]
    return [1, 16, 150, n]


PROGRAMS = ["keccak", "memory", "shared", "acc"] + [str(i) for i in sf.CASES]


def _all_cases():
    for name in PROGRAMS:
        for cap in _caps(name):
            yield name, cap


@functools.lru_cache(maxsize=None)
def _split(name, cap):
    from plonky2_gpu_amd.stark import StarkDesc, split_program

    instrs, imms, ncol, npi = _program(name)
    desc = StarkDesc(3, ncol, npi, 3, 2, si.fri_params(rate_bits=1), instrs, imms)
    return split_program(desc, cap)


def _is_emit(instrs):
    return np.isin(np.asarray(instrs)[:, 0], list(KINDS))


PARAMS = [pytest.param(name, cap, id="%s-cap%d" % (name, cap)) for name, cap in _all_cases()]


# ---------------------------------------------------------------- 1. properties
def test_the_keccak_program_is_the_long_one():
    instrs = _program("keccak")[0]
    assert len(instrs) == 47227 and int(_is_emit(instrs).sum()) == 842


@pytest.mark.parametrize("name,cap", PARAMS)
def test_units_partition_the_emits_validate_and_respect_the_cap(name, cap):
    instrs, imms, ncol, npi = _program(name)
    units = _split(name, cap)
    emits = instrs[_is_emit(instrs)]
    at = 0
    for k, (unit, (first, last)) in enumerate(units):
        assert first == at and last > first, (k, first, last, at)
        own = unit[_is_emit(unit)]
        assert len(own) == last - first and (own == emits[first:last]).all(), k  # the run, in order, operand for operand
        assert _is_emit(unit[-1:]).all(), k  # nothing behind the last EMIT
        sr.validate_program(unit, imms, ncol, npi)
        assert len(unit) <= cap or last - first == 1, (k, len(unit), cap)
        at = last
    assert at == len(emits)
    if cap >= len(instrs):
        assert len(units) == 1 and units[0][0].shape == instrs.shape and (units[0][0] == instrs).all()


def test_a_small_cap_cuts_and_a_unit_grows_while_it_fits():
    """the cuts are greedy: unit k + 1's first constraint did not fit into unit k"""
    for name, cap in (("keccak", 250), ("keccak", 1500), ("shared", 9), ("5", 16), ("11", 150)):
        units = _split(name, cap)
        assert len(units) > 1, (name, cap)
        grown = _split(name, 10 ** 6 if name == "keccak" else len(_program(name)[0]))
        assert len(grown) == 1
    # 12 constraints of 4 instructions that share instruction 0: at cap 9 two constraints fit (1 + 4 + 4), at cap 6 one
    assert [last - first for _, (first, last) in _split("shared", 9)] == [2] * 6
    assert [len(u) for u, _ in _split("shared", 9)] == [9] * 6
    assert [len(u) for u, _ in _split("shared", 6)] == [5] * 12
    assert all((u[0] == (sr.LOAD_WIRE, 7, 0, 0)).all() for u, _ in _split("shared", 6))


def test_an_acc_chain_across_a_cut_is_kept_whole():
    units = _split("acc", 1)
    assert [r for _, r in units] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    ops = lambda u: [tuple(int(x) for x in row) for row in u]  # noqa: E731
    assert ops(units[0][0]) == [(sr.LOAD_WIRE, 0, 0, 0), (sr.EMIT, 0, 0, 0)]  # the ACC in front of it feeds nothing it reads
    third = ops(units[2][0])
    assert [i for i in third if i[0] == sr.ACC and i[1] == 1] == [(sr.ACC, 1, 0, 0), (sr.ACC, 1, 2, 1), (sr.ACC, 1, 4, 2)]
    # accumulator 0: the first sum was read (and zeroed) by a dropped ACCR, so only the ACC behind that one is kept
    assert [i for i in third if i[0] == sr.ACC and i[1] == 0] == [(sr.ACC, 0, 2, 0)]
    assert (sr.ACCR, 3, 0, 0) not in third and (sr.LOAD_IMM, 9, 1, 0) not in ops(units[3][0])


# ---------------------------------------------------------------- 2. semantics
class _Recorder:
    """a ConstraintConsumer that keeps (kind, value)"""

    def __init__(self):
        self.emitted = []

    def constraint(self, c):
        self.emitted.append(("constraint", int(c) % P))

    def constraint_transition(self, c):
        self.emitted.append(("transition", int(c) % P))

    def constraint_first_row(self, c):
        self.emitted.append(("first_row", int(c) % P))

    def constraint_last_row(self, c):
        self.emitted.append(("last_row", int(c) % P))


def _rows(name, count):
    """`count` (local, next, public inputs) of any u64 words: field data with half of the liftable words lifted by p"""
    _, _, ncol, npi = _program(name)
    rng = np.random.default_rng(len(name) + 31 * ncol)
    words = rep.lift(rep.field_data(rng, (count, 2 * ncol + npi)), rng)[0]
    return [([int(x) for x in w[:ncol]], [int(x) for x in w[ncol:2 * ncol]], [int(x) for x in w[2 * ncol:]]) for w in words]


@functools.lru_cache(maxsize=None)
def _expected(name, count):
    instrs, imms, _, _ = _program(name)
    out = []
    for local, nxt, pis in _rows(name, count):
        rec = _Recorder()
        sr.run_program(sr.Base, instrs, imms, local, nxt, pis, rec)
        out.append(rec.emitted)
    return out


@pytest.mark.parametrize("name,cap", PARAMS)
def test_units_in_order_emit_what_the_program_emits(name, cap):
    instrs, imms, _, _ = _program(name)
    count = 2 if name == "keccak" else 3
    units = _split(name, cap)
    for (local, nxt, pis), exp in zip(_rows(name, count), _expected(name, count)):
        rec = _Recorder()
        for unit, _ in units:
            sr.run_program(sr.Base, unit, imms, local, nxt, pis, rec)
        assert len(exp) == int(_is_emit(instrs).sum()) and rec.emitted == exp


# ---------------------------------------------------------------- 3. device-free compile
COMPILED = [i for i in sf.CASES if sf.LENGTHS[i] == 400 and not any(sf.fuzz_case(i)["stark"].pairs)][0]

CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import stark_fuzz as sf, stark_ref as sr
import test_gpu_stark_fuzz as tgsf
import plonky2_gpu_amd as pg
from plonky2_gpu_amd import stark as pstark

units_cache, single_cache, empty = sys.argv[2], sys.argv[3], sys.argv[4]
case = sf.fuzz_case(int(sys.argv[5]))
desc = tgsf._desc(case)

def state(cache):
    return {f: os.stat(os.path.join(cache, f)).st_mtime_ns for f in sorted(os.listdir(cache))}

out = dict(devices=pg.load().gl_device_count())
os.environ["PLONKY2_HIP_KERNEL_CACHE"] = units_cache
units = pstark.split_program(desc, 100)
out["units"] = len(units)
out["distinct"] = len({u.tobytes() for u, _ in units})
pstark.precompile(desc, unit_instrs=100)
first = state(units_cache)
pstark.precompile(desc, unit_instrs=100)
out["new"], out["unchanged"] = sorted(first), state(units_cache) == first
out["sizes"] = {f: os.path.getsize(os.path.join(units_cache, f)) for f in first}

os.environ["PLONKY2_HIP_KERNEL_CACHE"] = single_cache
pstark.precompile(desc)
out["single_today"] = sorted(state(single_cache))
pstark.precompile(desc, unit_instrs=None)
out["single_none"] = sorted(state(single_cache))
pstark.precompile(desc, unit_instrs=10 ** 6)  # one unit of the whole program: the single kernel's source
out["single_large_cap"] = sorted(state(single_cache))

os.environ["PLONKY2_HIP_KERNEL_CACHE"] = empty
refused = None
for mutant, instrs, imms in tgsf._mutants(200, seed=4242):
    s = mutant["stark"]
    try:
        sr.validate_program(instrs, imms, s.num_columns, s.num_public_inputs)
        continue
    except ValueError:
        pass
    results = []
    for call in (lambda d: pstark.precompile(d, unit_instrs=16), lambda d: pstark.precompile(d, unit_instrs=0), lambda d: pstark.split_program(d, 16)):
        try:
            call(tgsf._desc(mutant, instrs, imms))
            results.append(None)
        except pg.Plonky2HipError as e:
            results.append(e.code)
    refused = results
    break
out["refused"], out["invalid"], out["empty_cache"] = refused, pg.GL_E_INVALID, sorted(os.listdir(empty))
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    base = tmp_path_factory.mktemp("stark_precompile_units")
    dirs = [base / name for name in ("units", "single", "empty")]
    for d in dirs:
        d.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLONKY2_HIP_")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD, HERE] + [str(d) for d in dirs] + [str(COMPILED)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_precompile_in_units_writes_one_kernel_per_unit_once(child):
    assert child["units"] > 3 and child["distinct"] == child["units"]  # distinct programs: distinct sources
    objects = [f for f in child["new"] if f.endswith(".hsaco")]
    assert len(objects) == child["units"], child
    assert all(f.startswith("stark_") and len(f) == len("stark_") + 16 + len(".hsaco") for f in objects)
    assert sorted(child["new"]) == sorted(objects + [f[:-6] + ".hip" for f in objects])  # no temporary file is left
    assert all(size > 1000 for size in child["sizes"].values())
    assert child["unchanged"]  # the second call wrote nothing


def test_precompile_without_a_cap_writes_the_single_kernel_it_always_wrote(child):
    assert len(child["single_today"]) == 2 and child["single_today"][0].endswith(".hip") and child["single_today"][1].endswith(".hsaco")
    assert child["single_none"] == child["single_today"] == child["single_large_cap"]
    assert not set(child["single_today"]) & set(child["new"])


def test_precompile_in_units_refuses_what_create_refuses_and_writes_nothing(child):
    assert child["refused"] == [child["invalid"]] * 3
    assert child["empty_cache"] == []
