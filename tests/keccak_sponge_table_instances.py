"""Inputs for the Keccak sponge table's tests (TEST INFRASTRUCTURE ONLY): deterministic operation lists, and the five-table system
of tests/test_keccak_sponge_table_ref.py and tests/test_gpu_keccak_sponge_table.py — the sponge, the Keccak-f, logic and memory
tables built from what the sponge makes them do, and a 14-column stand-in for the CPU table that looks up the sponge's outputs."""
import numpy as np

import keccak_sponge_table_ref as kr

LENGTHS = [0, 1, 3, 4, 134, 135, 136, 137, 271, 272, 273, 408]  # around one, two and three blocks; 135: both padding bits in one byte


def data(length, seed):
    return np.random.default_rng(1000 * seed + length).integers(0, 256, size=length, dtype=np.uint8).tobytes()


def op(length, k=0):
    """operation number k of a list: its own context, segment, address and timestamp"""
    return kr.KeccakSpongeOp(k, (3 * k + 1) % 7, 1000 * k + 17, 5 * k + 2, data(length, k))


def single(length):
    return [op(length)]


def mixed():
    """every length of LENGTHS in one list: 12 operations, 22 rows"""
    return [op(length, k) for k, length in enumerate(LENGTHS)]


def many(num_ops):
    """num_ops operations of lengths that cycle through LENGTHS"""
    return [op(LENGTHS[(5 * k) % len(LENGTHS)], k) for k in range(num_ops)]


# ---------------------------------------------------------------- the system
SYSTEM_LENGTHS = (140, 300)  # 2 + 3 = 5 sponge rows, final remainders 4 and 28
SPONGE, KECCAK, LOGIC, MEMORY, CPU = range(5)  # the tables' numbers
SYSTEM_DEGREE_BITS = {SPONGE: 3, KECCAK: 7, LOGIC: 5, CPU: 2}  # the memory table's comes from its row count
CPU_COLUMNS, CPU_FILTER = 14, 13


def system_ops():
    """Two operations in contexts 0 and 1. The memory table's value constraints are plain constraints that also tie its last row to
    row 0 (a read of an unchanged address sees the value of the row before; the last row's flags are zero): with reads alone, the
    byte at the largest address must be the byte at the smallest, so the last byte of the second input repeats the first of the
    first."""
    inputs = [bytearray(data(length, 40 + k)) for k, length in enumerate(SYSTEM_LENGTHS)]
    inputs[-1][-1] = inputs[0][0]
    return [kr.KeccakSpongeOp(k, kr.SEGMENT_CODE, 64 + 1000 * k, 8 * (k + 3), bytes(b)) for k, b in enumerate(inputs)]


class CpuStandIn:
    """the 14-column stand-in for the CPU table in ctl_keccak_sponge: context, segment, virt, len, timestamp, the eight output limbs
    and a filter; its own constraint: the filter is boolean"""
    num_columns, num_public_inputs, constraint_degree, pairs = CPU_COLUMNS, 0, 3, []

    def __init__(self):
        from plonky2_gpu_amd.stark import StarkAsm

        a = StarkAsm()
        f = a.local(CPU_FILTER)
        a.emit(a.mul(f, a.sub(f, a.imm(1))))
        self.instrs, self.immediates = a.program()

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        consumer.constraint(F.mul(local[CPU_FILTER], F.sub(local[CPU_FILTER], F.one)))


def cpu_trace(operations):
    """[14][4]: one filtered row per operation — what the CPU table holds after KECCAK_GENERAL: the address, the length, the time and
    Keccak-256 of the input as eight little-endian u32s — then rows of sevens under a filter of 0"""
    import keccak_ref

    rows = []
    for o in operations:
        digest = keccak_ref.keccak256(o.input)
        rows.append([o.context, o.segment, o.virt, len(o.input), o.timestamp] + [int.from_bytes(digest[4 * j : 4 * j + 4], "little") for j in range(8)] + [1])
    while len(rows) < 4:
        rows.append([7] * 13 + [0])
    assert len(rows) == 4
    return [[r[c] for r in rows] for c in range(CPU_COLUMNS)]


class System:
    def __init__(self, tables, lookups):
        self.tables, self.lookups, self.ctl_closures = tables, lookups, None


WITHOUT_KECCAK = {"sponge": 0, "logic": 1, "memory": 2, "cpu": 3}  # the tables' numbers in the four-table system
ALL_FIVE = {"sponge": SPONGE, "keccak": KECCAK, "logic": LOGIC, "memory": MEMORY, "cpu": CPU}


def lookups(which=("keccak", "logic", "memory", "sponge"), xored=True, logic_filter="rows", memory_strict=True, numbers=None):
    """the sponge's four cross-table lookups over the tables' numbers (`numbers`: name -> number, default the five above).
    xored / logic_filter ("rows": ctl_looking_logic_filter(), "reference": ctl_looking_memory_filter(i)) / memory_strict choose
    between the reference's words and the descriptions that hold."""
    from plonky2_gpu_amd import keccak_sponge_table as ks
    from plonky2_gpu_amd import keccak_table as kt
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd import memory_table as mt
    from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, TableWithColumns

    t = ALL_FIVE if numbers is None else numbers
    out = []
    if "keccak" in which:
        out.append(CrossTableLookup([TableWithColumns(t["sponge"], ks.ctl_looking_keccak(xored=xored), ks.ctl_looking_keccak_filter())],
                                    TableWithColumns(t["keccak"], kt.ctl_data(), kt.ctl_filter())))
    if "logic" in which:
        flt = (lambda i: ks.ctl_looking_logic_filter()) if logic_filter == "rows" else (lambda i: ks.ctl_looking_memory_filter(i))
        out.append(CrossTableLookup([TableWithColumns(t["sponge"], ks.ctl_looking_logic(i), flt(i)) for i in range(ks.num_logic_ctls())],
                                    TableWithColumns(t["logic"], lt.ctl_data(), lt.ctl_filter())))
    if "memory" in which:
        out.append(CrossTableLookup([TableWithColumns(t["sponge"], ks.ctl_looking_memory(i), ks.ctl_looking_memory_filter(i, strict=memory_strict))
                                     for i in range(ks.KECCAK_RATE_BYTES)],
                                    TableWithColumns(t["memory"], mt.ctl_data(), mt.ctl_filter())))
    if "sponge" in which:
        out.append(CrossTableLookup([TableWithColumns(t["cpu"], [CtlColumn.single(c) for c in range(13)], CtlColumn.single(CPU_FILTER))],
                                    TableWithColumns(t["sponge"], ks.ctl_looked_data(), ks.ctl_looked_filter())))
    return out
