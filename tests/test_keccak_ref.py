"""tests/keccak_ref.py — the numpy Keccak every GPU test of the Keccak trees is held against — pinned three ways (this image's
hashlib has no Keccak-256 and the reference ships no vector), and the Keccak entry points at the library's boundary: declared in
the header, exported, bound in _lib.py. No GPU is needed: argument refusals are tested on the GPU (without a device there is no
context, and every call is refused for that reason alone)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import keccak_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = kr.P
SYMBOLS = ["gl_keccak_hash_no_pad_batch", "gl_merkle_tree_from_columns_h", "gl_merkle_tree_from_leaves_h", "gl_commit_from_coeffs_h",
           "gl_commit_from_values_h"]


@pytest.mark.parametrize("length", [0, 1, 8, 135, 136, 137, 271, 272, 1080, 5000])
def test_with_the_sha3_padding_byte_it_is_hashlib_sha3_256(length):
    """same permutation, same rate; only the padding byte differs"""
    rng = np.random.default_rng(1000 + length)
    msgs = rng.integers(0, 256, size=(5, length), dtype=np.uint8)
    got = kr.keccak256_batch(msgs, pad_byte=0x06)
    for m, g in zip(msgs, got):
        assert g.tobytes() == hashlib.sha3_256(m.tobytes()).digest()
    assert kr.keccak256(msgs[0].tobytes(), pad_byte=0x06) == hashlib.sha3_256(msgs[0].tobytes()).digest()


def test_published_keccak256_values():
    assert kr.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert kr.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


FIELD_ANSWERS = [
    ([], "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7b"),
    ([0], "011b4d03dd8c01f1049143cf9c4c817e4b167f1d1b83e5c6f0"),
    (list(range(17)), "c8aaeb4115ae34eaedae3ec43b06fca7b23728e5f7a6b90454"),  # one full block + the padding block
    (list(range(135)), "7c32392ed88b3e8f7fecbb97580a206ef8eb3262e7df9ac546"),
    ([P - 1] * 5, "1abe8018043cfdbce92b7a16f367ff07834dea697b7469e7cf"),
]
TWO_TO_ONE_ZEROS = "767bfb6ead6760f170718f8074950b9439f9d58e73b64f2554"


@pytest.mark.parametrize("x,answer", FIELD_ANSWERS)
def test_hash_no_pad_known_answers(x, answer):
    got = kr.hash_no_pad(np.array(x, dtype=np.uint64).reshape(1, -1))
    assert got.shape == (1, 25) and got[0].tobytes().hex() == answer


def test_two_to_one_known_answer():
    z = np.zeros((1, 25), dtype=np.uint8)
    assert kr.two_to_one(z, z)[0].tobytes().hex() == TWO_TO_ONE_ZEROS
    assert kr.two_to_one(z, z)[0].tobytes() == kr.keccak256(bytes(50))[:25]


def test_inputs_are_reduced_before_they_are_absorbed():
    a = np.array([[P + 5, 2**64 - 1, P, 1, 2]], dtype=np.uint64)
    b = np.array([[5, 2**32 - 2, 0, 1, 2]], dtype=np.uint64)
    assert (kr.hash_no_pad(a) == kr.hash_no_pad(b)).all()


def test_hash_or_noop():
    x = np.array([[P + 1, 2, 3]], dtype=np.uint64)
    for k in range(4):
        h = kr.hash_or_noop(x[:, :k])
        assert h.shape == (1, 25)
        assert h[0].tobytes() == b"".join(int(v % P).to_bytes(8, "little") for v in x[0, :k].tolist()) + bytes(25 - 8 * k)
    with pytest.raises(ValueError):
        kr.hash_or_noop(np.zeros((1, 4), dtype=np.uint64))
    y = np.arange(5, dtype=np.uint64).reshape(1, 5)
    assert (kr.hash_or_noop(y) == kr.hash_no_pad(y)).all()


def test_slots_and_back():
    h = np.random.default_rng(3).integers(0, 256, size=(7, 25), dtype=np.uint8)
    s = kr.slots(h)
    assert s.shape == (7, 4) and s.dtype == np.uint64 and (s[:, 3] < 256).all()
    assert (kr.hash_bytes(s) == h).all()
    s[2, 3] |= np.uint64(1 << 8)
    with pytest.raises(AssertionError):
        kr.hash_bytes(s)


def _tree_by_recursion(hashes):
    """MerkleTree::fill_subtree (merkle_tree.rs:78-105) word for word: returns (digest list, root)"""
    if len(hashes) == 1:
        return [], hashes[0]
    half = len(hashes) // 2
    ld, lr = _tree_by_recursion(hashes[:half])
    rd, rr = _tree_by_recursion(hashes[half:])
    root = kr.two_to_one(lr.reshape(1, 25), rr.reshape(1, 25))[0]
    return ld + [lr, rr] + rd, root


@pytest.mark.parametrize("n,leaf_len,cap_height", [(16, 7, 0), (16, 3, 2), (8, 5, 3), (32, 20, 1), (1, 9, 0)])
def test_merkle_tree_layout_is_the_recursive_one_and_proofs_verify(n, leaf_len, cap_height):
    rng = np.random.default_rng(n * 100 + leaf_len)
    leaves = rng.integers(0, 2**64, size=(n, leaf_len), dtype=np.uint64)
    digests, cap = kr.merkle_tree(leaves, cap_height)
    hashes = list(kr.hash_or_noop(leaves))
    per = n >> cap_height
    exp_d, exp_c = [], []
    for s in range(1 << cap_height):
        d, r = _tree_by_recursion(hashes[s * per:(s + 1) * per])
        exp_d += d
        exp_c.append(r)
    assert digests.shape == (2 * (n - (1 << cap_height)), 25) and cap.shape == (1 << cap_height, 25)
    assert (cap == np.array(exp_c)).all()
    if exp_d:
        assert (digests == np.array(exp_d)).all()
    # MerkleTree::prove (merkle_tree.rs:392-440) on that array, verified like merkle_proofs.rs:57-86
    layers = (n.bit_length() - 1) - cap_height
    tree_len = 2 * (per - 1)
    for i in range(n):
        pair, sib = i & (per - 1), []
        for l in range(layers):
            parity, pair = pair & 1, pair >> 1
            sib.append(digests[tree_len * (i >> layers) + 2 * ((pair << (l + 1)) + (1 << l) - 1) + (1 - parity)])
        assert kr.merkle_verify(leaves[i], i, cap, np.array(sib).reshape(layers, 25))
        assert kr.merkle_verify_batch(leaves[i:i + 1], [i], cap, np.array(sib).reshape(1, layers, 25)).all()
    if layers:
        bad = np.array(sib).reshape(layers, 25).copy()
        bad[0, 0] ^= 1
        assert not kr.merkle_verify(leaves[n - 1], n - 1, cap, bad)


# ---- the boundary of the library ------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky2_hip.h")).read(), flags=re.S)


def test_keccak_symbols_are_declared_exported_and_bound():
    from plonky2_gpu_amd import _lib

    text = _header()
    lib_path = os.path.join(ROOT, "plonky2_gpu_amd", "libplonky2_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(rf"^\s*GlError\s+{name}\s*\(", text, flags=re.M), f"{name} is not declared in plonky2_hip.h"
        assert re.search(rf"\bT {name}$", exported, flags=re.M), f"{name} is not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.GlError
        f = getattr(lib, name)
        assert f.restype is _lib.GlError and list(f.argtypes) == list(args)
    # the `_h` calls are the un-suffixed ones with the hasher in front
    for name in SYMBOLS[1:]:
        assert _lib.SIGNATURES[name][1] == [ctypes.c_uint32] + _lib.SIGNATURES[name[:-2]][1]
        m = re.search(rf"GlError\s+{name}\s*\(([^;]*)\);", text)
        plain = re.search(rf"GlError\s+{name[:-2]}\s*\(([^;]*)\);", text)
        assert " ".join(m.group(1).split()) == "uint32_t hasher, " + " ".join(plain.group(1).split())


def test_hasher_constants_match_the_header():
    from plonky2_gpu_amd import _lib

    m = re.search(r"enum GlHasher \{(.*?)\}", _header(), flags=re.S)
    assert m, "enum GlHasher is not in plonky2_hip.h"
    values = {k: int(v) for k, v in re.findall(r"(GL_HASHER_\w+)\s*=\s*(\d+)", m.group(1))}
    assert values == {"GL_HASHER_POSEIDON": 0, "GL_HASHER_KECCAK25": 1}
    for k, v in values.items():
        assert getattr(_lib, k) == v
    assert _lib.hasher_id("poseidon") == _lib.GL_HASHER_POSEIDON and _lib.hasher_id("keccak") == _lib.GL_HASHER_KECCAK25
    with pytest.raises(ValueError):
        _lib.hasher_id("sha256")


def test_without_a_context_every_keccak_call_is_refused():
    """a NULL context is GL_E_INVALID before anything touches a device"""
    from plonky2_gpu_amd import _lib

    lib = _lib.load()
    for hasher in (_lib.GL_HASHER_POSEIDON, _lib.GL_HASHER_KECCAK25, 7):
        for name, args in [("gl_merkle_tree_from_columns_h", (hasher, None, 5, 8, 8, 0, None, None, None)),
                           ("gl_merkle_tree_from_leaves_h", (hasher, None, 5, 8, 0, None, None, None)),
                           ("gl_commit_from_coeffs_h", (hasher, None, 5, 3, 1, 0, 0, 7, None, None, None, None, None)),
                           ("gl_commit_from_values_h", (hasher, None, 5, 3, 1, 0, 0, 7, None, None, None, None, None))]:
            err = getattr(lib, name)(*args)
            assert err.code == _lib.GL_E_INVALID, (name, hasher)
            with pytest.raises(_lib.Plonky2HipError):
                _lib.check(err)
    err = lib.gl_keccak_hash_no_pad_batch(None, 0, 0, 1, None, None)
    assert err.code == _lib.GL_E_INVALID
    with pytest.raises(_lib.Plonky2HipError):
        _lib.check(err)


# ---- conditions on the kernels and the documents that need no GPU -------------------------------------------------------------

def test_no_keccak_kernel_uses_scratch(tmp_path):
    """the state is 50 VGPRs: a spill would mean the rounds were not unrolled into registers"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "plonky2_gpu_amd", "csrc", "keccak.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "keccak.co")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) == len(scratch) == 3 and all("keccak" in k for k in kernels), kernels
    assert scratch == [0, 0, 0], list(zip(kernels, scratch))


def test_the_documents_quote_the_committed_keccak_measurement():
    """profiles/keccak_commit.json is what tools/bench_keccak_commit.py wrote on the MI355X; the gate held there, and the tables
    of DESIGN.md and the paragraph of README.md carry its medians"""
    import json

    res = json.loads(open(os.path.join(ROOT, "profiles", "keccak_commit.json")).read())
    assert res["gate"] is True and [s["rows"] for s in res["sizes"]][0] == "2^20"
    design, readme = (open(os.path.join(ROOT, d)).read() for d in ("DESIGN.md", "README.md"))
    for s in res["sizes"]:
        assert s["reps"] >= 7 and s["keccak"]["median_ms"] <= s["poseidon"]["median_ms"]
        for h in ("poseidon", "keccak"):
            assert "%.2f ms" % s[h]["median_ms"] in design, (s["rows"], h)
            assert "%.1f" % s[h]["median_ms"] in readme, (s["rows"], h)
