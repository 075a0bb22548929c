"""The reference verifier (tests/stark_ref.py) on the bytes of a device STARK proof, for the tools that make acceptance their exit
condition (tools/bench_keccak_table.py --compiled): the checker lives under tests/, a tool only calls it."""
import generic_prove_ref as gr
import stark_ref as sr
import stark_scale as ss
from oracle import accel
from plonky2_gpu_amd import stark as pstark


def accepts(desc, data):
    """True if sr.verify accepts the Poseidon proof `data` of the StarkDesc `desc` (it raises AssertionError where it does not)"""
    parsed = pstark.proof_from_bytes(data, desc)
    with accel.c_backend():
        return sr.verify(gr.PoseidonHasher(), ss.RefStark(desc), desc.num_challenges, desc.fri_params, parsed) is True
