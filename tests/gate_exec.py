"""The gate register programs executed with Python integers (TEST INFRASTRUCTURE ONLY): a direct reading of the opcode definitions
in include/plonky2_hip.h, including the two halves of an ACC accumulator and the bound both must respect. Shared by
tests/test_gate_programs_cpu.py (the emitters against the oracle's gates) and tests/gate_fuzz.py (the reference of the raw programs)."""
from plonky2_gpu_amd import gate_program as gp

P = 0xFFFFFFFF00000001


def execute(instrs, imms, num_selectors, consts, wires, pih, open_accumulators=False):
    """one gate's program on one row -> the list of emitted constraint values (mod p, or the raw word of a register that was only
    loaded). Inputs may be any u64 words. Accumulators start at zero; one that is left unreduced at the end is an error unless
    `open_accumulators` (the header allows it: "Accumulators start at 0 in every gate")."""
    regs, out = {}, []
    acc_lo, acc_hi = [0] * 4, [0] * 4
    execute.worst = [0] * 4
    for op, dst, a, b in instrs:
        if op == gp.LOAD_WIRE:
            regs[dst] = wires[a]
        elif op == gp.LOAD_CONST:
            regs[dst] = consts[num_selectors + a]
        elif op == gp.LOAD_PI:
            regs[dst] = pih[a]
        elif op == gp.LOAD_IMM:
            regs[dst] = imms[a] % P
        elif op == gp.ADD:
            regs[dst] = (regs[a] + regs[b]) % P
        elif op == gp.SUB:
            regs[dst] = (regs[a] - regs[b]) % P
        elif op == gp.MUL:
            regs[dst] = regs[a] * regs[b] % P
        elif op == gp.MULK:
            regs[dst] = (regs[a] << b) % P
        elif op == gp.EMIT:
            out.append(regs[a])
        elif op == gp.ACC:
            # registers hold ANY u64 representative on the device: take the worst case for the bound, 2^32 - 1 per half
            assert imms[b] < 1 << 32
            x = regs[a]
            acc_lo[dst] += (x & 0xFFFFFFFF) * imms[b]
            acc_hi[dst] += (x >> 32) * imms[b]
            execute.worst[dst] += 0xFFFFFFFF * imms[b]
            assert execute.worst[dst] < 1 << 63, "an accumulator half could wrap"
        elif op == gp.ACCR:
            regs[dst] = (acc_lo[a] + (acc_hi[a] << 32)) % P
            acc_lo[a] = acc_hi[a] = 0
            execute.worst[a] = 0
        else:
            raise AssertionError("unknown opcode %d" % op)
    assert open_accumulators or (acc_lo == [0] * 4 and acc_hi == [0] * 4), "an accumulator was left unreduced"
    return out


execute.worst = [0] * 4
