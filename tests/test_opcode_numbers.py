"""The register-program opcodes are numbered in one place per language: csrc/program_isa.h for the library (its static_asserts tie
the enum to the numbers), and on the Python side gate_program.py, stark.py and tests/stark_ref.py; tests/gate_exec.py takes
gate_program's. They agree with each other and with 0..14 as include/plonky2_hip.h documents them."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)  # the helper modules of tests/, as the other tests reach them

import gate_exec  # noqa: E402
import stark_ref  # noqa: E402
from plonky2_gpu_amd import gate_program, stark  # noqa: E402

NAMES = ["LOAD_WIRE", "LOAD_CONST", "LOAD_PI", "LOAD_IMM", "ADD", "SUB", "MUL", "EMIT", "MULK", "ACC", "ACCR", "LOAD_NEXT", "EMIT_TRANSITION",
         "EMIT_FIRST_ROW", "EMIT_LAST_ROW"]
GATE_NAMES = NAMES[:11]


def _documented():
    """name -> the numbers the public header gives it ("  9 ACC  acc[dst] += ...", "4 ADD  5 SUB  6 MUL")"""
    text = open(os.path.join(ROOT, "include", "plonky2_hip.h")).read()
    pair = r"(\d+) (%s)\b" % "|".join(sorted(NAMES, key=len, reverse=True))
    found = {}
    for line in text.splitlines():
        if re.match(r" \*\s+" + pair, line):  # a line of one of the two opcode tables begins with an entry
            for number, name in re.findall(r"(?<![\w.])" + pair, line):
                found.setdefault(name, set()).add(int(number))
    return found


def test_opcode_numbers_agree_with_each_other_and_with_the_public_header():
    documented = _documented()
    for number, name in enumerate(NAMES):
        assert documented.get(name) == {number}, (name, documented.get(name))
        assert getattr(stark_ref, name) == number, name
        assert getattr(stark, name) == number, name
    for number, name in enumerate(GATE_NAMES):
        assert getattr(gate_program, name) == number, name
    assert gate_exec.gp is gate_program  # the executor of the tests has no numbers of its own: it reads gate_program's
    assert stark.EMITS == (7, 12, 13, 14)
