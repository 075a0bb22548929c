"""gl_stark_precompile / gl_stark_tables_precompile without a device: a description is validated as gl_stark_create /
gl_stark_tables_create validate it, its quotient kernel is generated (csrc/stark_jit.hip) and compiled by hiprtc into the kernel
cache — what a build machine without a GPU runs so that gl_stark_compile finds its kernels.

Everything the library does here happens in ONE child process whose PLONKY2_HIP_KERNEL_CACHE is a temporary directory (the shipped
cache is a build product); the tests read what it reports. It compiles the three hand-written STARKs of tests/stark_instances.py,
two 60-instruction descriptions of tests/stark_fuzz.py and the three tables of tests/ctl_instances.py: eight hiprtc compilations
of two to three seconds each."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import stark_fuzz as sf  # noqa: E402

FUZZ = [i for i in sf.CASES if sf.LENGTHS[i] == 60]

CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import ctl_instances as ci, stark_fuzz as sf, stark_instances as si, stark_ref as sr
import test_gpu_stark_fuzz as tgsf
import plonky2_gpu_amd as pg
from plonky2_gpu_amd import stark as pstark

cache, empty, listing = sys.argv[2], sys.argv[3], sys.argv[4]
os.environ["PLONKY2_HIP_KERNEL_CACHE"] = cache
os.environ["PLONKY2_HIP_KERNEL_CACHE_LIST"] = listing

def state():
    return {f: os.stat(os.path.join(cache, f)).st_mtime_ns for f in sorted(os.listdir(cache))}

def listed():
    paths = open(listing).read().split() if os.path.exists(listing) else []
    open(listing, "w").close()
    return [os.path.basename(p) for p in paths]

def twice(desc, hasher="poseidon"):
    before = state()
    pstark.precompile(desc, hasher)
    first, names = state(), listed()
    pstark.precompile(desc, hasher)
    second, again = state(), listed()
    return dict(new=sorted(set(first) - set(before)), listed=names, listed_again=again, unchanged=first == second,
                sizes={f: os.path.getsize(os.path.join(cache, f)) for f in set(first) - set(before)})

out = dict(devices=pg.load().gl_device_count(), singles={}, fuzz={})
for name in ("A", "B", "C"):
    out["singles"][name] = twice(si.STARKS[name].desc(3, 2, si.fri_params(rate_bits=2)))
fuzz = [i for i in sf.CASES if sf.LENGTHS[i] == 60]
with_pairs = [i for i in fuzz if any(sf.fuzz_case(i)["stark"].pairs)]
without = [i for i in fuzz if i not in with_pairs]
for i in (with_pairs[0], (without or with_pairs[1:])[0]):
    case = sf.fuzz_case(i)
    out["fuzz"][str(i)] = dict(twice(tgsf._desc(case)), pairs=case["stark"].pairs)
out["tables"] = twice(ci.system(3).desc(ci.DEGREE_BITS, 2, ci.fri_params(rate_bits=1)))
out["tables"]["num_tables"] = 3

# refusals: into an empty cache that has to stay empty
os.environ["PLONKY2_HIP_KERNEL_CACHE"] = empty
refused = []
for case, instrs, imms in tgsf._mutants(200, seed=4242):
    s = case["stark"]
    try:
        sr.validate_program(instrs, imms, s.num_columns, s.num_public_inputs)
        continue
    except ValueError as e:
        want = str(e)
    try:
        pstark.precompile(tgsf._desc(case, instrs, imms))
        refused.append(dict(reference=want, code=None, message=None))
    except pg.Plonky2HipError as e:
        refused.append(dict(reference=want, code=e.code, message=str(e)))
    if len(refused) == 10:
        break
out["mutants"] = refused
try:
    pstark.precompile(si.A.desc(4, 2, si.fri_params(arity_bits=(2,))), "keccak")  # 4 trace columns
    out["keccak"] = dict(code=None, message=None)
except pg.Plonky2HipError as e:
    out["keccak"] = dict(code=e.code, message=str(e))
out["invalid"] = pg.GL_E_INVALID
out["empty_cache"] = sorted(os.listdir(empty))
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    base = tmp_path_factory.mktemp("stark_precompile")
    cache, empty = base / "cache", base / "empty"
    cache.mkdir()
    empty.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLONKY2_HIP_")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD, HERE, str(cache), str(empty), str(base / "list.txt")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _written_once(entry, kernels):
    """`kernels` new code objects, each with its source beside it, all listed; the second call wrote nothing and listed the same"""
    objects = [f for f in entry["new"] if f.endswith(".hsaco")]
    assert len(objects) == kernels and all(f.startswith("stark_") and len(f) == len("stark_") + 16 + len(".hsaco") for f in objects), entry
    assert sorted(entry["new"]) == sorted(objects + [f[:-6] + ".hip" for f in objects]), entry  # no temporary file is left
    assert all(entry["sizes"][f] > 1000 for f in entry["new"]), entry
    assert sorted(entry["listed"]) == sorted(f[:-6] for f in objects) == sorted(entry["listed_again"]), entry
    assert entry["unchanged"], entry


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_precompile_writes_the_kernel_of_a_hand_written_stark_once(child, name):
    _written_once(child["singles"][name], 1)


def test_the_three_hand_written_starks_have_three_kernels(child):
    assert len({f for e in child["singles"].values() for f in e["new"]}) == 6


def test_precompile_writes_the_kernels_of_two_fuzz_descriptions_once(child):
    assert len(child["fuzz"]) == 2 and all(int(i) in FUZZ for i in child["fuzz"])
    assert sorted(bool(any(e["pairs"])) for e in child["fuzz"].values())[-1] is True  # one of them with permutation pairs
    for entry in child["fuzz"].values():
        _written_once(entry, 1)


def test_tables_precompile_writes_one_kernel_per_distinct_table_source(child):
    """the three tables of tests/ctl_instances.py differ in program and lookups: three sources, three kernels"""
    entry = child["tables"]
    _written_once(entry, len(set(entry["listed"])))
    assert len(set(entry["listed"])) == entry["num_tables"] == 3


def test_precompile_refuses_what_create_refuses_and_writes_nothing(child):
    """ten mutants tests/stark_ref.py's validate_program refuses, and the Keccak leaf of four elements"""
    assert len(child["mutants"]) == 10
    for m in child["mutants"]:
        assert m["code"] == child["invalid"] and m["message"] and m["message"].strip(), m
    assert child["keccak"]["code"] == child["invalid"] and "4 elements" in child["keccak"]["message"], child["keccak"]
    assert child["empty_cache"] == []
