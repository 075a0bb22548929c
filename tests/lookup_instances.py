"""The STARK "L" as data (TEST INFRASTRUCTURE, in the shape of tests/stark_instances.py): a range check by the Halo2-style lookup
argument of the reference (evm/src/lookup.rs; its use in memory_stark.rs:147 and :452-456).

L  6 columns, no public inputs, degree 3 (qdf 2, qdb 1):
     c0  a counter: first row 0, c0' = c0 + 1 — the table 0 .. n - 1
     v   the values under the range check, every one in [0, n), with a seeded-random multiplicity: about half of the counter's
         values never occur, the others up to many times
     pv, pt   permuted_cols(v, c0), constrained by eval_lookups
     f4  f4' = f4 + c0          f5  f5' = f5 + v pv pt (degree 3)
   The two fillers keep every oracle's leaf away from 4 elements (KeccakHash<25> cannot hash those). The permutation pairs are
   lookup_pairs' [(v, pv)] and [(c0, pt)]; the program comes from StarkAsm.eval_lookups, the closure is written by hand."""
import numpy as np

import lookup_ref
from plonky2_gpu_amd.lookup import lookup_pairs
from plonky2_gpu_amd.stark import StarkAsm
from stark_instances import TestStark

P = 0xFFFFFFFF00000001
C0, V, PV, PT, F4, F5 = range(6)
LOOKUPS = [(V, C0, PV, PT)]  # (input, table, permuted input, permuted table)
# With qdf 2, two challenges give four quotient polynomials: a leaf KeccakHash<25> cannot hash. Three give 6, and 3 Zs.
NUM_CHALLENGES = {"poseidon": 2, "keccak": 3}


def l_program():
    a = StarkAsm()
    a.emit_first_row(a.local(C0))
    a.emit_transition(a.sub(a.next(C0), a.add(a.local(C0), a.imm(1))))
    a.release()
    a.eval_lookups(PV, PT)
    a.release()
    a.emit_transition(a.sub(a.sub(a.next(F4), a.local(F4)), a.local(C0)))
    a.emit_transition(a.sub(a.sub(a.next(F5), a.local(F5)), a.mul(a.mul(a.local(V), a.local(PV)), a.local(PT))))
    return a


def l_closure(F, local, nxt, pis, c):
    c.constraint_first_row(local[C0])
    c.constraint_transition(F.sub(nxt[C0], F.add(local[C0], F.one)))
    diff_input_prev = F.sub(nxt[PV], local[PV])  # lookup.rs:24
    diff_input_table = F.sub(nxt[PV], nxt[PT])  # :26
    c.constraint(F.mul(diff_input_prev, diff_input_table))
    c.constraint_last_row(diff_input_table)
    c.constraint_transition(F.sub(F.sub(nxt[F4], local[F4]), local[C0]))
    c.constraint_transition(F.sub(F.sub(nxt[F5], local[F5]), F.mul(F.mul(local[V], local[PV]), local[PT])))


def l_values(degree_bits, seed=0):
    """the column v: n values drawn from a random half of [0, n)"""
    n = 1 << degree_bits
    rng = np.random.default_rng(1000 + seed)
    allowed = rng.permutation(n)[: max(1, n // 2)]
    return [int(x) for x in allowed[rng.integers(0, len(allowed), size=n)]]


def l_trace_from_values(v, fill=True):
    """the six columns around a given column v; fill=False leaves pv and pt zero (and f5 as if they were filled), for the device to
    fill them"""
    n = len(v)
    c0 = list(range(n))
    pv, pt = lookup_ref.permuted_cols(v, c0)
    f4, f5 = [3], [5]
    for r in range(n - 1):
        f4.append((f4[r] + c0[r]) % P)
        f5.append((f5[r] + v[r] % P * pv[r] % P * pt[r]) % P)
    zero = [0] * n
    return [c0, list(v), pv if fill else zero, pt if fill else list(zero), f4, f5]


def _l_trace(degree_bits, seed=0):
    return l_trace_from_values(l_values(degree_bits, seed)), []


L = TestStark("L", 6, 0, 3, lookup_pairs(LOOKUPS), l_program(), l_closure, _l_trace)
