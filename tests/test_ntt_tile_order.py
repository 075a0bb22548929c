"""The tile walk of the two direct NTT passes (tests/ntt_tile_order_model.py): every tile exactly once in either sweep direction.
CPU only."""
import itertools
import os
import re

import pytest

import ntt_tile_order_model as m

GX = [1, 64, 128, 300]
GY = [1, 3, 18, 64, 65]
GZ = [1, 8]
CUS = [64, 256]
SHAPES = list(itertools.product(GX, GY, GZ, CUS))


def _walks(kind, gx, gy, gz, cus, down):
    if kind in ("col", "coset"):
        W, per_b = m.col_launch(gx, gy, gz, cus)
        return [m.col_tiles(blk, W, gx, gy, gz, per_b, down, coset=kind == "coset") for blk in range(W)]
    W = m.row_launch(gx, gy, gz, cus)
    return [m.row_tiles(blk, W, gx, gy, gz, down) for blk in range(W)]


# the coset pass needs a workgroup to keep its column tile (per_b != 0): the launcher refuses the other grids
CASES = [(k,) + s for k in ("col", "coset", "row") for s in SHAPES if k != "coset" or m.col_launch(s[0], s[1], s[2], s[3])[1]]


@pytest.mark.parametrize("kind,gx,gy,gz,cus", CASES)
def test_every_tile_once_in_both_directions(kind, gx, gy, gz, cus):
    every = sorted(itertools.product(range(gx), range(gy), range(gz)))
    up = _walks(kind, gx, gy, gz, cus, False)
    down = _walks(kind, gx, gy, gz, cus, True)
    for walks in (up, down):
        seen = sorted(t for w in walks for t in w)
        assert seen == every
    # the downward walk is the upward one with the polynomial mirrored, workgroup by workgroup and step by step: column tile and
    # block stay (the column pass's kept twiddles and the row pass's store addresses depend on them alone)
    for wu, wd in zip(up, down):
        assert [(b, gy - 1 - a, z) for b, a, z in wu] == wd
    if gy > 1:
        assert up != down


def test_model_matches_the_source():
    src = open(os.path.join(os.path.dirname(__file__), "..", "plonky2_gpu_amd", "csrc", "ntt_direct.hip")).read()
    assert len(re.findall(r"if \(p\.sweep_down\) a = gy - 1 - a;", src)) == 2  # tile_of of both kernels
