"""What tests/test_gpu_stark_scale.py needs beside itself (TEST INFRASTRUCTURE): the adaptor from the library's descriptions to the
objects tests/stark_ref.py and tests/ctl_ref.py evaluate, the `counter` STARK whose trace numpy builds without a loop, and the list of
sizes the module proves.

The shapes themselves are the benchmarks' own (tools/bench_stark_prove.py, tools/bench_keccak_table.py): the proofs checked are the
proofs measured."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_keccak_table as bkt  # noqa: E402,F401
import bench_stark_prove as bsp  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import stark_ref as sr  # noqa: E402
from oracle import fri_ref  # noqa: E402

from plonky2_gpu_amd import stark as pstark  # noqa: E402

P = 0xFFFFFFFF00000001


# ---------------------------------------------------------------- descriptions as the reference takes them
class RefStark:
    """a StarkDesc as the object sr.verify / sr.prove evaluate with evaluator="program": shape, pairs and the register program.
    There is no hand-written closure: the verifier runs the program the device ran, over the extension field, in Python."""
    closure = None

    def __init__(self, desc):
        self.num_columns, self.num_public_inputs, self.constraint_degree = desc.num_columns, desc.num_public_inputs, desc.constraint_degree
        self.pairs = [list(pair) for pair in desc.pairs]
        # plain tuples of ints: the interpreter of tests/stark_ref.py walks them
        self.instrs, self.immediates = [tuple(int(x) for x in row) for row in desc.instrs], [int(x) for x in desc.immediates]


class RefSystem:
    """a StarkTablesDesc as the object cr.verify_tables evaluates; the lookups are the description's own objects (looking_tables,
    looked_table, default; table, columns, filter_column; terms, constant)"""
    ctl_closures = None

    def __init__(self, tables_desc):
        self.tables, self.lookups = [RefStark(d) for d in tables_desc.tables], list(tables_desc.lookups)


# ---------------------------------------------------------------- Keccak Merkle paths, all queries at once
class KeccakAtOnce(gr.KeccakHasher):
    """KeccakHasher with a memo from exact inputs to their hash, filled for the Merkle paths of all of a proof's queries level by
    level: keccak_ref.hash_or_noop / two_to_one on 84 rows at once instead of on one row 84 times. A 2430-element leaf is 143 sponge
    blocks; row by row the numpy sponge takes 26 s to verify a proof of the Keccak table under Keccak trees, at once under a second.
    The memo only ever holds H(input) as the same functions compute it, and what it does not hold is hashed as before: the
    verifier runs unchanged and its verdict cannot differ."""

    def __init__(self):
        self.leaves, self.nodes, self.hits = {}, {}, 0

    def remember_paths(self, paths):
        """`paths`: (leaf, index, siblings) of one tree: leaves of one length, paths of one length"""
        cur = self.hash_or_noop_batch([leaf for leaf, _, _ in paths])
        for (leaf, _, _), h in zip(paths, cur):
            self.leaves[tuple(int(x) for x in leaf)] = h
        idx = [i for _, i, _ in paths]
        for level in range(len(paths[0][2])):
            sib = [bytes(p[2][level]) for p in paths]
            lefts = [s if i & 1 else c for s, c, i in zip(sib, cur, idx)]
            rights = [c if i & 1 else s for s, c, i in zip(sib, cur, idx)]
            cur = self.two_to_one_batch(lefts, rights)
            self.nodes.update(zip(zip(lefts, rights), cur))
            idx = [i >> 1 for i in idx]

    def remember_fri_proof(self, opening_proof, query_indices, arity_bits):
        rounds = opening_proof["query_round_proofs"]
        for k in range(len(rounds[0]["initial_trees_proof"])):
            self.remember_paths([(rp["initial_trees_proof"][k][0], x, rp["initial_trees_proof"][k][1]) for x, rp in zip(query_indices, rounds)])
        shift = 0
        for i, ab in enumerate(arity_bits):
            shift += ab
            self.remember_paths([(fri_ref.flatten(rp["steps"][i]["evals"]), x >> shift, rp["steps"][i]["merkle_proof"]) for x, rp in zip(query_indices, rounds)])

    def hash_or_noop(self, inputs):
        key = tuple(int(x) for x in inputs)
        if key in self.leaves:
            self.hits += 1
            return self.leaves[key]
        return super().hash_or_noop(inputs)

    def two_to_one(self, left, right):
        key = (bytes(left), bytes(right))
        if key in self.nodes:
            self.hits += 1
            return self.nodes[key]
        return super().two_to_one(left, right)


def keccak_at_once(stark, num_challenges, fri_params, proof):
    """a KeccakAtOnce that remembers the paths of `proof` (a parsed single-table proof); the query indices are the verifier's own"""
    hasher = KeccakAtOnce()
    lde_bits = fri_params["cap_height"] + len(proof["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"][0][1])
    chal = sr.get_challenges(hasher, stark, num_challenges, fri_params, proof, lde_bits - fri_params["rate_bits"])
    hasher.remember_fri_proof(proof["opening_proof"], chal["fri_challenges"]["fri_query_indices"], fri_params["reduction_arity_bits"])
    return hasher


# ---------------------------------------------------------------- counter: four columns, numpy only
COUNTER_START = 7


def counter_program():
    """c0 starts at pi[0] and counts; c1 = c0^2 on every row (degree 2: qdf 1, qdb 0); columns 2 and 3 one permutation pair"""
    a = pstark.StarkAsm()
    c0 = a.local(0)
    a.emit_first_row(a.sub(c0, a.pi(0)))
    a.emit_transition(a.sub(a.next(0), a.add(c0, a.imm(1))))
    a.emit(a.sub(a.local(1), a.mul(c0, c0)))
    return a.program()


def counter_trace(degree_bits):
    """([4][n] uint64, public inputs). c0 < 2^24 + 7, so c0^2 < 2^49 needs no reduction; column 3 is column 2 rotated by one row."""
    n = 1 << degree_bits
    trace = np.empty((4, n), dtype=np.uint64)
    trace[0] = np.arange(COUNTER_START, n + COUNTER_START, dtype=np.uint64)
    trace[1] = trace[0] * trace[0]
    trace[2] = np.arange(n, dtype=np.uint64)
    trace[3] = np.roll(trace[2], 1)
    return trace, [COUNTER_START]


def counter_desc(degree_bits):
    instrs, imms = counter_program()
    return pstark.StarkDesc(degree_bits, 4, 1, 2, 2, bsp.fast_config_fri_params(degree_bits), instrs, imms, [[(2, 3)]])


def counter(ctx, degree_bits):
    """(description, trace in HBM, public inputs), as tools/bench_stark_prove.py's fibonacci and wide return them"""
    import plonky2_gpu_amd as pg

    trace, pis = counter_trace(degree_bits)
    return counter_desc(degree_bits), pg.DeviceBuffer.from_host(ctx, trace), pis


MAKERS = {"fibonacci": bsp.fibonacci, "wide": bsp.wide, "counter": counter}

# (shape, degree_bits) of the single-table proofs the reference verifier must accept; rate_bits is 1 in standard_fast_config, so the LDE
# (one NTT per column, and the FRI domain) has 2^(degree_bits + 1) points
ACCEPTED = [("fibonacci", 12), ("fibonacci", 16), ("fibonacci", 20), ("wide", 12), ("wide", 16), ("counter", 21), ("counter", 22), ("counter", 23)]
COMPILED = [c for c in ACCEPTED if c[0] in ("fibonacci", "wide")]
KECCAK_TABLE = [(12, "poseidon", 2), (14, "poseidon", 2), (12, "keccak", 1)]  # degree_bits, hasher, challenges
