"""The order in which the workgroups of the two direct NTT passes walk their tiles (csrc/ntt_direct.hip: tile_of of
ntt_col_direct_kernel and of ntt_row_natural_direct_kernel, the launchers' grids), restated in Python by hand: nothing but a count of
the source's mirroring line ties it to the kernels, so it documents the walk and checks the ARITHMETIC of the restatement (grid
rounding, per_b dealing, the XCD map); that the kernels compute the same is what tests/test_gpu_ntt_sweep.py holds on the device.
tests/test_ntt_tile_order.py checks on it:

  * every tile (b, a, z) of a launch is taken by exactly one workgroup exactly once, whichever way the pass sweeps
    (PassParams::sweep_down maps the polynomial a -> gy - 1 - a for loads and stores alike: the same bijection).

A tile is (b, a, z): column / row tile b of polynomial a of block z (grid x, y, z of the launch)."""

def xcd_map(block, W):
    """workgroups of one XCD (block % 8) take adjacent tiles"""
    return (block & 7) * (W >> 3) + (block >> 3) if (W & 7) == 0 else block


def col_launch(gx, gy, gz, cus):
    """launch_col_direct_t: (workgroups, per_b)"""
    pairs = gy * gz
    if gx <= cus:
        per_b = min(cus // gx, pairs)
        return gx * per_b, per_b
    return cus, 0


def col_tiles(block, W, gx, gy, gz, per_b, sweep_down=False, coset=False):
    """the tiles of workgroup `block` of the column pass, in the order it walks them; coset: the first pass of the LDE (z = coset,
    the per_b workgroups of a column tile are neighbours and a workgroup takes the cosets of a polynomial one after the other)"""
    u = xcd_map(block, W)
    P = gy * gz
    if per_b:
        b0, p0 = (u // per_b, u % per_b) if coset else (u % gx, u // gx)
        bstep, pstep = gx, per_b
    else:
        b0, p0, bstep, pstep = u, 0, W, 1
    np_local = (P - p0 + pstep - 1) // pstep if p0 < P else 0
    nb_local = (gx - b0 + bstep - 1) // bstep if b0 < gx else 0
    out = []
    for t in range(np_local * nb_local):
        bi, pi = divmod(t, np_local)
        pp = p0 + pi * pstep
        a, z = (pp // gz, pp % gz) if coset else (pp % gy, pp // gy)
        if sweep_down:
            a = gy - 1 - a
        out.append((b0 + bi * bstep, a, z))
    return out


def row_launch(gx, gy, gz, cus):
    """launch_row_natural_direct_t: workgroups"""
    return min(gx * gy * gz, cus)


def row_tiles(block, W, gx, gy, gz, sweep_down=False):
    """the tiles of workgroup `block` of the natural-order row pass, in the order it walks them"""
    u = xcd_map(block, W)
    total = gx * gy * gz
    if u >= total:
        return []
    out = []
    for t in range((total - u + W - 1) // W):
        ident = u + t * W
        b, r = ident % gx, ident // gx
        a, z = r % gy, r // gy
        if sweep_down:
            a = gy - 1 - a
        out.append((b, a, z))
    return out
