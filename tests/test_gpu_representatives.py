"""Every field entry point with NON-CANONICAL representatives (include/plonky2_hip.h, Conventions: inputs may be any u64
representative, outputs are canonical). A Rust host hands the library unreduced words: plonky2's GoldilocksField arithmetic
returns sums and products >= p as they are (goldilocks_field.rs: Add, reduce128).

For every case, with a copy of the input in which liftable words x < 2^32 - 1 became x + p (tests/representatives.py), and
host scalars lifted too (2^64 - 1 and 2^64 - 2 among them):
  (a) the output for the lifted input equals the output for the canonical input, bit for bit;
  (b) the canonical output equals the big-integer reference the entry point's own test uses;
  (c) every output word is < p.
Data are mostly small values, so that lifting reaches most entries, and the rare paths of the field operations fire:
gl::add's second wrap (both operands >= p), gl::sub's second borrow (minuend < 2^32, subtrahend > p), the lazy dot
products' carry counters (long sums of words with large halves). The kernels reach them through the lifted device data;
most host scalars (betas, gammas, alphas, the coset shift, evaluation points) are reduced on the host before a launch, and
lifting them checks that reduction.

The pass-through entry points (gl_transpose, gl_ext2_interleave, gl_pack_leaf_ranges, the opened leaves of
gl_merkle_open_batch{,_device}) move words and are pinned as such: the output holds the input's words unchanged."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from gpu_util import P, bitrev_perm, gpu  # noqa: F401
from representatives import LIFTABLE, all_canonical, field_data, lift, lift_scalar

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
# canonical scalars whose lifted forms are 2^64 - 1 and 2^64 - 2
TOP, TOP2 = (1 << 32) - 2, (1 << 32) - 3


def _lib():
    from plonky2_gpu_amd import _lib

    return _lib


def _buf(gpu, a):
    import plonky2_gpu_amd as pg

    return pg.DeviceBuffer.from_host(gpu, np.ascontiguousarray(a, dtype=np.uint64).reshape(-1))


def _zeros(gpu, n):
    import plonky2_gpu_amd as pg

    b = pg.DeviceBuffer(gpu, max(n, 1))
    _lib().call("gl_memset_zero", b.ptr, 8 * max(n, 1), gpu.ptr)
    return b


def _ext_lists(planar):
    a = np.asarray(planar, dtype=np.uint64).reshape(2, -1)
    return [(int(x), int(y)) for x, y in zip(a[0], a[1])]


def _check(lifted_out, canon_out):
    """(a) and (c)"""
    lifted_out, canon_out = np.asarray(lifted_out, dtype=np.uint64), np.asarray(canon_out, dtype=np.uint64)
    assert all_canonical(canon_out), "canonical input gave a non-canonical output"
    assert all_canonical(lifted_out), "non-canonical input gave a non-canonical output"
    assert lifted_out.shape == canon_out.shape and (lifted_out == canon_out).all(), "output depends on the representative"


# ---- FRI primitives ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n,m,extreme", [(0, 1, False), (10, 64, False), (12, 300, False), (8, 520, False), (8, 520, True)])
def test_reduce_polys_base(gpu, log_n, m, extreme):
    from oracle import fri_ref

    rng = np.random.default_rng(100 + log_n * 1000 + m + extreme)
    n = 1 << log_n
    if extreme:  # every word 2^64 - 1 or p - 1: both halves of every term near 2^32, the DotAcc carry counters at their limit
        pick = rng.random((m, n)) < 0.5
        polys = np.where(pick, np.uint64(TOP), np.uint64(P - 1)).astype(np.uint64)
        lifted = np.where(pick, np.uint64(M64), np.uint64(P - 1)).astype(np.uint64)
        count = int(pick.sum())
        alpha = (TOP, TOP)
    else:
        polys = field_data(rng, (m, n))
        polys[0, 0] = TOP
        lifted, count = lift(polys, rng, 0.6)
        lifted[0, 0], count = M64, count + int(lifted[0, 0] == TOP)
        alpha = [(TOP, TOP2), (5, P - 1), (int(rng.integers(0, LIFTABLE)), int(rng.integers(0, LIFTABLE)))][(log_n + m) % 3]
    assert count > m * n // 4
    outs = []
    for data, a in ((polys, alpha), (lifted, tuple(lift_scalar(x) for x in alpha))):
        d = _buf(gpu, data)
        d_ptrs = _buf(gpu, np.array([d.ptr + 8 * n * j for j in range(m)], dtype=np.uint64))
        d_out = _zeros(gpu, 2 * n)
        _lib().call("gl_fri_reduce_polys_base", d_ptrs.ptr, m, n, np.array(a, dtype=np.uint64), d_out.ptr, gpu.ptr)
        outs.append(d_out.download())
    _check(outs[1], outs[0])
    got = _ext_lists(outs[0])
    cols = sorted(set([0, n - 1] + [int(i) for i in rng.integers(0, n, size=min(n, 24))]))
    exp = fri_ref.reduce_polys_base([[int(p[i]) for i in cols] for p in polys], alpha)
    assert [got[i] for i in cols] == exp


@pytest.mark.parametrize("log_n", [1, 10, 11, 18])  # inside one 1024-element scan block, exactly one, two, many
def test_divide_by_linear(gpu, log_n):
    from oracle import fri_ref

    rng = np.random.default_rng(200 + log_n)
    n = 1 << log_n
    total = 0
    for acc in (0, 1):
        comp = field_data(rng, (2, n))
        prior = field_data(rng, (2, n))
        if acc:
            z, scale = (TOP, 3), (TOP2, TOP)
        else:
            z, scale = (int(rng.integers(0, LIFTABLE)), TOP2), (1, 0)
        l_comp, c1 = lift(comp, rng, 0.6)
        l_prior, c2 = lift(prior, rng, 0.6)
        total += c1 + c2
        outs = []
        for cm, pr, zz, sc in ((comp, prior, z, scale), (l_comp, l_prior, tuple(map(lift_scalar, z)), tuple(map(lift_scalar, scale)))):
            d_c, d_f = _buf(gpu, cm), _buf(gpu, pr)
            _lib().call("gl_fri_divide_by_linear", d_c.ptr, n, np.array(zz, dtype=np.uint64), np.array(sc, dtype=np.uint64), acc,
                        d_f.ptr, gpu.ptr)
            outs.append(d_f.download())
        _check(outs[1], outs[0])
        q = fri_ref.divide_by_linear(_ext_lists(comp), z)
        pr = _ext_lists(prior)
        exp = [(0, 0)] + [fri_ref.ext_add(fri_ref.ext_mul(pr[i + 1], scale) if acc else (0, 0), q[i]) for i in range(n - 1)]
        assert _ext_lists(outs[0]) == exp, acc
    assert total > n


@pytest.mark.parametrize("log_len,ab", [(1, 1), (4, 2), (6, 3), (10, 4), (14, 1), (14, 4), (18, 4), (19, 2)])
def test_fold_fold_device_and_interleave(gpu, log_len, ab):
    """gl_fri_fold with lifted coefficients and beta (also beta = p, i.e. zero: out[k] is the caller's word c[k*arity]; and
    1 + p); gl_fri_fold_device with the same coefficients and the canonical beta in device memory (as documented);
    gl_ext2_interleave moves the caller's words unchanged."""
    from oracle import fri_ref

    rng = np.random.default_rng(300 + log_len * 10 + ab)
    n = 1 << log_len
    coeffs = field_data(rng, (2, n))
    lifted, count = lift(coeffs, rng, 0.7)
    assert count > n // 2
    d_c, d_l = _buf(gpu, coeffs), _buf(gpu, lifted)
    ext = _ext_lists(coeffs)
    ks = sorted(set([0, (n >> ab) - 1] + [int(k) for k in rng.integers(0, n >> ab, size=16)]))
    for beta in ((TOP, TOP2), (0, 0), (1, 0), (int(rng.integers(0, LIFTABLE)), 7)):
        lb = tuple(map(lift_scalar, beta))  # (0, 0) -> (p, p), (1, 0) -> (1 + p, p)
        outs = []
        for d, b in ((d_c, beta), (d_l, lb)):
            d_o = _zeros(gpu, 2 * (n >> ab))
            _lib().call("gl_fri_fold", d.ptr, n, ab, np.array(b, dtype=np.uint64), d_o.ptr, gpu.ptr)
            outs.append(d_o.download())
        _check(outs[1], outs[0])
        got = _ext_lists(outs[0])
        for k in ks:
            assert got[k] == fri_ref.reduce_with_powers_ext(ext[k << ab : (k + 1) << ab], beta), (beta, k)
        d_beta = _buf(gpu, np.array(beta, dtype=np.uint64))
        d_o = _zeros(gpu, 2 * (n >> ab))
        _lib().call("gl_fri_fold_device", d_l.ptr, n, ab, d_beta.ptr, d_o.ptr, gpu.ptr)
        _check(d_o.download(), outs[0])
    # pass-through: rows[2i + c] = plane_c[i], the words themselves
    d_r = _zeros(gpu, 2 * n)
    _lib().call("gl_ext2_interleave", d_l.ptr, n, d_r.ptr, gpu.ptr)
    assert (d_r.download() == lifted.T.reshape(-1)).all()


@pytest.mark.parametrize("log_n", [0, 4, 12, 16])
def test_eval_polys_ext2(gpu, log_n):
    """points 0, 1, X, p - 1, their lifted forms and random ones, one to four at a time, column stride > 2^log_n. At log_n 0 or
    at the point 0 the result is a caller word."""
    from oracle import plonk_ref

    rng = np.random.default_rng(400 + log_n)
    n = 1 << log_n
    poly_num, stride = 5, n + 3
    coeffs = field_data(rng, (poly_num, n))
    lifted, count = lift(coeffs, rng, 0.7)
    assert count >= poly_num * n // 3
    pad = lambda a: np.concatenate([a, np.full((poly_num, stride - n), 0xDEAD, dtype=np.uint64)], axis=1)  # noqa: E731
    d_c, d_l = _buf(gpu, pad(coeffs)), _buf(gpu, pad(lifted))
    r = lambda: int(rng.integers(0, LIFTABLE))  # noqa: E731
    pts = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (TOP, TOP2), (r(), r()), (int(rng.integers(0, P, dtype=np.uint64)), r())]
    sample = [0, poly_num - 1] if n > 4096 else range(poly_num)
    for num_points in (1, 2, 3, 4):
        for start in range(0, len(pts), num_points):
            chosen = (pts + pts)[start : start + num_points]
            outs = []
            for d, pp in ((d_c, chosen), (d_l, [tuple(map(lift_scalar, q)) for q in chosen])):
                d_o = _zeros(gpu, 2 * num_points * poly_num)
                _lib().call("gl_eval_polys_ext2", d.ptr, poly_num, log_n, stride, np.array(pp, dtype=np.uint64).reshape(-1),
                            num_points, d_o.ptr, gpu.ptr)
                outs.append(d_o.download())
            _check(outs[1], outs[0])
            if num_points == 4 or n <= 16:
                got = outs[0].reshape(num_points, poly_num, 2)
                for q, z in enumerate(chosen):
                    for i in sample:
                        assert tuple(int(v) for v in got[q, i]) == plonk_ref.eval_ext2([int(c) for c in coeffs[i]], z), (q, i)


# ---- the permutation argument and the quotient -------------------------------------------------------------------------

@pytest.mark.parametrize("num_routed,degree_bits,qdf,num_ch", [(10, 4, 8, 2), (80, 6, 8, 2), (9, 11, 4, 3)])
def test_partial_products(gpu, num_routed, degree_bits, qdf, num_ch):
    """wires (small witness values) and sigmas lifted, k_0 = 1 as 1 + p, betas / gammas among them 2^64 - 1 and 2^64 - 2.
    The host reduces betas and gammas before the launch, so the kernel only ever adds a canonical gamma: lifting them checks
    that reduction; the lifted words the kernel itself sees are the wires, sigmas and k_is."""
    from oracle import plonk_ref, pyref

    rng = np.random.default_rng(500 + num_routed + degree_bits)
    n = 1 << degree_bits
    wires_stride = n + 5
    wires = field_data(rng, (num_routed + 2, n), small=0.85)
    sigmas = field_data(rng, (num_routed, n), small=0.5)
    k_is = np.array([pow(pyref.GENERATOR, j, P) for j in range(num_routed)], dtype=np.uint64)
    betas = [TOP, TOP2, 5][:num_ch]
    gammas = [TOP2, TOP, int(rng.integers(0, LIFTABLE))][:num_ch]
    l_w, c1 = lift(wires, rng, 0.8)
    l_s, c2 = lift(sigmas, rng, 0.8)
    l_k = np.array([lift_scalar(k) for k in k_is], dtype=np.uint64)
    assert c1 > wires.size // 2 and c2 > 0 and int(l_k[0]) == 1 + P
    n_cols = num_ch * (1 + plonk_ref.num_partial_products(num_routed, qdf))
    outs = []
    for w, s, k, b, g in ((wires, sigmas, k_is, betas, gammas), (l_w, l_s, l_k, [lift_scalar(x) for x in betas], [lift_scalar(x) for x in gammas])):
        wpad = np.concatenate([w, np.full((w.shape[0], wires_stride - n), 0xBAD, dtype=np.uint64)], axis=1)
        d_w, d_s, d_k = _buf(gpu, wpad), _buf(gpu, s), _buf(gpu, k)
        d_o = _zeros(gpu, n_cols * n)
        _lib().call("gl_permutation_partial_products", d_w.ptr, wires_stride, d_s.ptr, n, d_k.ptr, np.array(b, dtype=np.uint64),
                    np.array(g, dtype=np.uint64), num_ch, num_routed, qdf, degree_bits, d_o.ptr, gpu.ptr)
        outs.append(d_o.download())
    _check(outs[1], outs[0])
    subgroup = [pow(pyref.root_of_unity(degree_bits), i, P) for i in range(n)]
    exp = plonk_ref.zs_partial_products(wires[:num_routed].tolist(), sigmas.tolist(), [int(k) for k in k_is], betas, gammas, qdf, subgroup)
    assert (outs[0].reshape(n_cols, n) == np.array(exp, dtype=np.uint64)).all()


def _quotient(gpu, d_w, d_cs, d_z, leaf_lens, column_stride, inst, k_is, betas, gammas, alphas, qdf, source, d_terms=None, prog=None,
              pih=None, shift=7):
    """gl_compute_quotient_polys on raw leaf buffers; source: none / terms / program / kernel"""
    _l = _lib()
    degree_bits, rate_bits = inst["degree_bits"], 3
    qdb = (qdf - 1).bit_length()
    b, g, a = (np.array(x, dtype=np.uint64) for x in (betas, gammas, alphas))
    d_k = _buf(gpu, k_is)
    size = b.size << (degree_bits + qdb)
    work = _zeros(gpu, size) if source == "kernel" else None
    h_pih = np.array(pih if pih is not None else [0] * 4, dtype=np.uint64)
    args = _l.GlQuotientArgs(
        d_w.ptr, d_cs.ptr, d_z.ptr, leaf_lens[0], leaf_lens[1], leaf_lens[2], d_k.ptr,
        d_terms.ptr if source == "terms" else None, b.ctypes.data, g.ctypes.data, a.ctypes.data,
        inst["num_constants"], inst["num_routed"], b.size, inst["num_gate_constraints"] if source != "none" else 0,
        degree_bits, rate_bits, qdf, shift,
        ctypes.pointer(prog.struct) if source == "program" else None, column_stride,
        prog.kernel if source == "kernel" else None, h_pih.ctypes.data if source == "kernel" else None,
        work.ptr if work is not None else None)
    out = _zeros(gpu, size)
    _l.call("gl_compute_quotient_polys", ctypes.byref(args), out.ptr, gpu.ptr)
    gpu.synchronize()
    return out.download()


@pytest.mark.parametrize("num_ch", [1, 2, 3, 4])
def test_compute_quotient_polys(gpu, num_ch):
    """all three leaf buffers lifted (selectors among them: the gate filter's sub(i, s) with s >= p is gl::sub's second borrow),
    k_is, alphas / betas / gammas, the gate terms and the public-inputs hash; every gate source (none: the fast kernels
    <num_challenges>; a term array, the interpreter, the compiled kernel: the generic kernel), leaf-major and column-major (at a
    column stride of n_ext and at a padded one), the coset shift given as 7 + p"""
    import plonky2_gpu_amd as pg
    from oracle import plonk_ref, pyref
    from plonky2_gpu_amd import gate_program as gp
    from plonk_instance import make_circuit_instance

    rng = np.random.default_rng(600 + num_ch)
    qdf, rate_bits = 8, 3
    inst = make_circuit_instance(degree_bits=4, seed=60 + num_ch, num_challenges=num_ch)
    n, nc, ngc = inst["n"], inst["num_constants"], inst["num_gate_constraints"]
    n_ext = n << rate_bits
    bits = 4 + rate_bits
    nz = num_ch * (1 + plonk_ref.num_partial_products(inst["num_routed"], qdf))
    # leaves [n_ext][leaf_len] in leaf order, made of small values; the selector column holds gate indices and UNUSED_SELECTOR
    w_l = field_data(rng, (n_ext, 12))
    cs_l = field_data(rng, (n_ext, nc + 12))
    cs_l[:, 0] = np.array([0, 1, 2, 3, 0, 3, plonk_ref.UNUSED_SELECTOR], dtype=np.uint64)[rng.integers(0, 7, size=n_ext)]
    z_l = field_data(rng, (n_ext, nz))
    k_is = np.array(inst["k_is"], dtype=np.uint64)
    betas, gammas, alphas = [TOP, 3, TOP2, 11][:num_ch], [TOP2, TOP, 0, 1][:num_ch], [TOP, 9, TOP2, 0][:num_ch]
    pih = [TOP, 0, 17, TOP2]
    terms = field_data(rng, (n_ext, ngc))
    lifted = {}
    count = 0
    for name, a in (("w", w_l), ("cs", cs_l), ("z", z_l), ("terms", terms)):
        lifted[name], c = lift(a, rng, 0.7)
        count += c
    assert count > (w_l.size + cs_l.size + z_l.size) // 2
    assert (lifted["cs"][:, 0] >= np.uint64(P)).sum() > n_ext // 4  # lifted selectors
    lk = np.array([lift_scalar(k) for k in k_is], dtype=np.uint64)
    lsc = lambda v: [lift_scalar(x) for x in v]  # noqa: E731
    gates = [gp.noop_gate(), gp.constant_gate(2), gp.public_input_gate(), gp.arithmetic_gate(3)]
    progs = {key: pg.GateProgram(gpu, gates, inst["selector_indices"], inst["groups"], h) for key, h in (("canon", pih), ("lifted", lsc(pih)))}
    kernel_prog = pg.GateProgram(gpu, gates, inst["selector_indices"], inst["groups"], [0] * 4).compile(ngc, num_ch)  # pih per call
    # the references
    w_rows, cs_rows, z_rows = w_l.tolist(), cs_l.tolist(), z_l.tolist()
    ref_args = (w_rows, cs_rows, z_rows, nc, [int(k) for k in k_is], betas, gammas, alphas, 4, rate_bits, qdf)
    gate_terms = [plonk_ref.evaluate_gate_constraints(inst["gates"], inst["selector_indices"], inst["groups"], ngc,
                                                      cs_rows[pyref.reverse_bits(i, bits)][:nc], w_rows[pyref.reverse_bits(i, bits)], pih)
                  for i in range(n_ext)]
    exp = {"none": plonk_ref.compute_quotient_polys(*ref_args), "terms": plonk_ref.compute_quotient_polys(*ref_args, terms.tolist()),
           "program": plonk_ref.compute_quotient_polys(*ref_args, gate_terms)}
    exp["kernel"] = exp["program"]
    for source in ("none", "terms", "program", "kernel"):
        for column_stride in (0, n_ext, n_ext + 2):  # n_ext + 2: a padded column pitch, the pad words no field elements
            outs = []
            for key in ("canon", "lifted"):
                lf = key == "lifted"
                bufs = [lifted[nm] if lf else a for nm, a in (("w", w_l), ("cs", cs_l), ("z", z_l))]
                if column_stride:
                    bufs = [np.concatenate([a.T, np.full((a.shape[1], column_stride - n_ext), 0xFFFFFFFFDEADBEEF, dtype=np.uint64)], axis=1)
                            for a in bufs]
                d = [_buf(gpu, a) for a in bufs]
                d_t = _buf(gpu, lifted["terms"] if lf else terms)
                outs.append(_quotient(gpu, d[0], d[1], d[2], (12, nc + 12, nz), column_stride, inst,
                                      lk if lf else k_is, lsc(betas) if lf else betas, lsc(gammas) if lf else gammas,
                                      lsc(alphas) if lf else alphas, qdf, source, d_terms=d_t,
                                      prog=kernel_prog if source == "kernel" else progs[key], pih=lsc(pih) if lf else pih,
                                      shift=7 + P if lf else 7))
            _check(outs[1], outs[0])
            assert (outs[0].reshape(num_ch, -1) == np.array(exp[source], dtype=np.uint64)).all(), (source, column_stride)


# ---- transforms and commitments ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n", [3, 12, 21])
def test_coset_transforms_with_a_lifted_shift(gpu, oracle, log_n):
    """gl_coset_ntt_batch forward and inverse and gl_coset_lde_batch with the values lifted and shift = 7 + p (also the key of
    the coset-table cache: 7 and 7 + p must give the same result), column stride > 2^log_n"""
    rng = np.random.default_rng(700 + log_n)
    n, polys = 1 << log_n, 2
    stride = 2 * n  # > 2^log_n, and a multiple of it as the inverse requires
    vals = field_data(rng, (polys, n))
    lifted, count = lift(vals, rng, 0.7)
    assert count > n // 2
    pad = lambda a: np.concatenate([a, np.zeros((polys, stride - n), dtype=np.uint64)], axis=1)  # noqa: E731
    for inverse in (0, 1):
        outs = []
        for data, shift in ((vals, 7), (lifted, 7 + P), (vals, 7 + P), (lifted, 7)):
            d = _buf(gpu, pad(data))
            _lib().call("gl_coset_ntt_batch", d.ptr, polys, log_n, stride, shift, inverse, gpu.ptr)
            outs.append(d.download().reshape(polys, stride)[:, :n])
        for o in outs[1:]:
            _check(o, outs[0])
        exp = oracle.canon(np.stack([oracle.coset_ifft(v) if inverse else oracle.coset_fft(v) for v in vals]))
        assert (outs[0] == exp).all(), inverse
    rate_bits = 1 if log_n == 21 else 3
    n_ext = n << rate_bits
    outs = []
    for data, shift in ((vals, 7), (lifted, 7 + P)):
        d, d_o = _buf(gpu, pad(data)), _zeros(gpu, polys * n_ext)
        _lib().call("gl_coset_lde_batch", d.ptr, d_o.ptr, polys, log_n, rate_bits, shift, stride, n_ext, gpu.ptr)
        outs.append(d_o.download().reshape(polys, n_ext))
    _check(outs[1], outs[0])
    exp = oracle.canon(oracle.coset_lde_batch(vals, rate_bits, threads=4))[:, bitrev_perm(log_n + rate_bits)]
    assert (outs[0] == exp).all()


def _commit(gpu, data, from_values, log_n, rate_bits, h, salt, leaf_major):
    """gl_commit_from_{values,coeffs}; returns (coefficients or None, d_lde, leaves or None, digests, cap) as host arrays"""
    poly_num = data.shape[0]
    ss = 0 if salt is None else salt.shape[0]
    n_ext = 1 << (log_n + rate_bits)
    width = poly_num + ss
    d_in = _buf(gpu, data)
    d_lde = _zeros(gpu, width * n_ext)
    if salt is not None:
        d_lde.upload(np.ascontiguousarray(salt), poly_num * n_ext)
    d_leaves = _zeros(gpu, n_ext * width) if leaf_major else None
    nd = 4 * 2 * (n_ext - (1 << h))
    d_dig, d_cap = _zeros(gpu, nd), _zeros(gpu, 4 << h)
    name = "gl_commit_from_values" if from_values else "gl_commit_from_coeffs"
    _lib().call(name, d_in.ptr, poly_num, log_n, rate_bits, h, ss, 7, d_lde.ptr, d_leaves.ptr if leaf_major else None, d_dig.ptr,
                d_cap.ptr, gpu.ptr)
    gpu.synchronize()
    return (d_in.download() if from_values else None, d_lde.download(), d_leaves.download() if leaf_major else None,
            d_dig.download(0, nd), d_cap.download())


@pytest.mark.parametrize("n_polys,log_n,rate_bits,h,leaf_major,salted", [
    (20, 9, 3, 4, True, False), (20, 9, 3, 2, False, True), (20, 9, 3, 4, True, True),  # one-shot
    (48, 13, 3, 4, True, False), (57, 13, 3, 2, False, False), (60, 13, 3, 3, False, True), (48, 13, 3, 4, False, True),  # pipelined
    (50, 13, 3, 4, True, True),
])
def test_commit_from_values_and_coeffs(gpu, oracle, n_polys, log_n, rate_bits, h, leaf_major, salted):
    """values / coefficients and salts lifted: coefficients, d_lde (its salt columns included: they are reduced in place),
    leaves, digests and cap as for the canonical input. With leaf_major and salted, the salt columns of the leaf-major copy
    are outputs too."""
    rng = np.random.default_rng(800 + n_polys + log_n + h)
    n_ext = 1 << (log_n + rate_bits)
    vals = field_data(rng, (n_polys, 1 << log_n))
    salt = field_data(rng, (4, n_ext)) if salted else None
    l_vals, c1 = lift(vals, rng, 0.7)
    l_salt, c2 = lift(salt, rng, 0.7) if salted else (None, 0)
    assert c1 > vals.size // 2 and (c2 > n_ext or not salted)
    for from_values in (True, False):
        a = _commit(gpu, vals, from_values, log_n, rate_bits, h, salt, leaf_major)
        b = _commit(gpu, l_vals, from_values, log_n, rate_bits, h, l_salt, leaf_major)
        for x, y in zip(b, a):
            if x is not None:
                _check(x, y)
        exp = (oracle.commit_from_values if from_values else oracle.commit_from_coeffs)(vals, rate_bits, h, threads=8)
        leaves = oracle.canon(exp["leaves"])
        if salted:
            leaves = np.concatenate([leaves, salt.T], axis=1)
            dig, cap = oracle.merkle_tree(leaves, h, threads=8)
        else:
            dig, cap = exp["digests"], exp["cap"]
        if from_values:
            assert (a[0].reshape(n_polys, -1) == oracle.canon(exp["coeffs"])).all()
        assert (a[1].reshape(-1, n_ext) == leaves.T).all()
        if leaf_major:
            assert (a[2].reshape(n_ext, -1) == leaves).all()
        assert (a[3].reshape(-1, 4) == oracle.canon(dig).reshape(-1, 4)).all() and (a[4].reshape(-1, 4) == oracle.canon(cap)).all()


@pytest.mark.parametrize("leaf_len", [1, 4, 5, 8, 135])
def test_merkle_trees_and_openings(gpu, oracle, leaf_len):
    """gl_merkle_tree_from_leaves / _columns with every liftable word lifted (leaf_len <= 4: the leaf digest is the leaf itself,
    hash_or_noop), cap height 0 and the maximum; the opened leaves of gl_merkle_open_batch{,_device} are the caller's words
    unchanged (pass-through), the siblings the canonical digests"""
    rng = np.random.default_rng(900 + leaf_len)
    log_leaves = 6
    n = 1 << log_leaves
    leaves = field_data(rng, (n, leaf_len), small=0.8)
    lifted, count = lift(leaves, rng, 1.0)
    assert count == int((leaves < np.uint64(LIFTABLE)).sum()) and count > leaves.size // 2
    idx = np.array([0, n - 1, 5, 5, n // 2, 33], dtype=np.uint64)
    for h in (0, log_leaves):
        dig, cap = oracle.merkle_tree(leaves, h, threads=4)
        dig, cap = oracle.canon(dig).reshape(-1), oracle.canon(cap).reshape(-1)
        nd = max(dig.size, 1)
        for data in (leaves, lifted):
            d_rows, d_dig, d_cap = _buf(gpu, data), _zeros(gpu, nd), _zeros(gpu, cap.size)
            _lib().call("gl_merkle_tree_from_leaves", d_rows.ptr, leaf_len, n, h, d_dig.ptr, d_cap.ptr, gpu.ptr)
            assert all_canonical(d_dig.download()) and all_canonical(d_cap.download())
            assert (d_cap.download() == cap).all() and (dig.size == 0 or (d_dig.download(0, dig.size) == dig).all())
            d_cols, d2, c2 = _buf(gpu, np.ascontiguousarray(data.T)), _zeros(gpu, nd), _zeros(gpu, cap.size)
            _lib().call("gl_merkle_tree_from_columns", d_cols.ptr, leaf_len, n, n, h, d2.ptr, c2.ptr, gpu.ptr)
            assert (c2.download() == cap).all() and (dig.size == 0 or (d2.download(0, dig.size) == dig).all())
            layers = log_leaves - h
            for d_src, rs, es in ((d_rows, leaf_len, 1), (d_cols, 1, n)):
                h_l = np.zeros(idx.size * leaf_len, dtype=np.uint64)
                h_s = np.zeros(max(idx.size * layers * 4, 1), dtype=np.uint64)
                _lib().call("gl_merkle_open_batch", d_src.ptr, rs, es, leaf_len, n, h, d_dig.ptr, idx, idx.size, h_l, h_s, gpu.ptr)
                assert (h_l.reshape(idx.size, leaf_len) == data[idx.astype(np.int64)]).all()
                d_idx, d_ol, d_os = _buf(gpu, idx), _zeros(gpu, idx.size * leaf_len), _zeros(gpu, idx.size * layers * 4)
                _lib().call("gl_merkle_open_batch_device", d_src.ptr, rs, es, leaf_len, n, h, d_dig.ptr, d_idx.ptr, idx.size, 0,
                            d_ol.ptr, d_os.ptr, gpu.ptr)
                assert (d_ol.download() == h_l).all()
                if layers:
                    assert all_canonical(h_s) and (d_os.download() == h_s).all()
                    for q, i in enumerate(idx):
                        assert oracle.merkle_verify(leaves[int(i)], int(i), cap.reshape(-1, 4), h_s.reshape(idx.size, layers, 4)[q])


def test_transpose_and_pack_leaf_ranges_move_the_words_unchanged(gpu):
    """gl_transpose and gl_pack_leaf_ranges are pure data movement: the caller's words, lifted or not, come out as they went in"""
    rng = np.random.default_rng(1000)
    for n_cols, n_rows in ((7, 1000), (135, 64), (3, 4096)):
        stride = n_rows + 24
        cols = field_data(rng, (n_cols, stride))
        lifted, count = lift(cols, rng, 0.8)
        assert count > cols.size // 3
        d_c, d_r = _buf(gpu, lifted), _zeros(gpu, n_rows * n_cols)
        _lib().call("gl_transpose", d_c.ptr, d_r.ptr, n_cols, n_rows, stride, gpu.ptr)
        assert (d_r.download().reshape(n_rows, n_cols) == lifted[:, :n_rows].T).all()
        world = 4
        per = n_rows // world
        d_o = _zeros(gpu, world * n_cols * per)
        _lib().call("gl_pack_leaf_ranges", d_c.ptr, stride, n_cols, per, world, d_o.ptr, gpu.ptr)
        exp = np.stack([lifted[:, q * per : (q + 1) * per] for q in range(world)])
        assert (d_o.download().reshape(world, n_cols, per) == exp).all()


# ---- the transcript ----------------------------------------------------------------------------------------------------

def test_sponge_absorb_and_proof_of_work(gpu, oracle):
    from oracle import pyref

    rng = np.random.default_rng(1100)
    state = field_data(rng, 12, small=0.9)
    inputs = field_data(rng, 8 * 5, small=0.9)
    l_state, c1 = lift(state, rng, 1.0)
    l_inputs, c2 = lift(inputs, rng, 1.0)
    assert c1 + c2 > 30
    outs = []
    for s, x in ((state, inputs), (l_state, l_inputs)):
        h = np.ascontiguousarray(s, dtype=np.uint64).copy()
        _lib().call("gl_sponge_absorb", h, np.ascontiguousarray(x), 5, gpu.ptr)
        outs.append(h)
    _check(outs[1], outs[0])
    ref = [int(v) for v in state]
    for b in range(5):
        ref[:8] = [int(v) for v in inputs[8 * b : 8 * b + 8]]
        ref = pyref.poseidon(ref)
    assert [int(v) for v in outs[0]] == ref
    # the proof of work: the same smallest witness for either representative of the state
    bits = 10
    min_lz = bits + (64 - P.bit_length())
    ws = []
    for s in (state, l_state):
        w = ctypes.c_uint64()
        _lib().call("gl_fri_proof_of_work", np.ascontiguousarray(s), 3, min_lz, ctypes.addressof(w), gpu.ptr)
        ws.append(w.value)
    assert ws[0] == ws[1]

    # the smallest: every candidate below it fails (the C oracle's permutation, about 2^bits of them)
    cand = np.tile(np.asarray(state, dtype=np.uint64), (ws[0] + 1, 1))
    cand[:, 3] = np.arange(ws[0] + 1, dtype=np.uint64)
    lz = [64 - int(oracle.canon(oracle.poseidon(c))[7]).bit_length() for c in cand]
    assert lz[-1] >= min_lz and max(lz[:-1], default=0) < min_lz


# ---- the reference's own symbols ---------------------------------------------------------------------------------------

def test_reference_symbols(gpu, oracle):
    """ifft, merkle_tree_from_coeffs and merkle_tree_from_values with lifted values in the region: the same region words as
    the canonical run (test_gpu_merkle.py::test_reference_abi_entry_points' size and layout)"""
    import plonky2_gpu_amd as pg

    L = _lib()
    polys, log_n, rate_bits, h = 20, 9, 3, 4
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    rng = np.random.default_rng(1200)
    vals = field_data(rng, (polys, n))
    lifted, count = lift(vals, rng, 0.7)
    assert count > vals.size // 2
    exp = oracle.commit_from_values(vals, rate_bits, h, threads=4)
    pad = polys * n_ext
    nd = 2 * (n_ext - (1 << h))
    total = 2 * pad + 4 * nd + 4 * (1 << h)
    n_inv = ctypes.c_uint64(P - ((P - 1) >> log_n))
    regions = {}
    for key, data in (("canon", vals), ("lifted", lifted)):
        ext = pg.DeviceBuffer(gpu, total)
        ext.upload(data, 0)
        L.call("ifft", ext.ptr, polys, n, log_n, None, ctypes.addressof(n_inv), gpu.ptr)
        coeffs = ext.download(0, polys * n)
        L.call("merkle_tree_from_coeffs", ext.ptr, ext.ptr, polys, n, log_n, None, None, None, rate_bits, 0, h, pad, gpu.ptr)
        ext2 = pg.DeviceBuffer(gpu, total)
        ext2.upload(data, 0)
        L.call("merkle_tree_from_values", ext2.ptr, ext2.ptr, polys, n, log_n, None, None, None, ctypes.addressof(n_inv), rate_bits,
               0, h, pad, gpu.ptr)
        regions[key] = (coeffs, ext.download(), ext2.download())
    for x, y in zip(regions["lifted"], regions["canon"]):
        _check(x, y)
    coeffs, region, region2 = regions["canon"]
    assert (coeffs.reshape(polys, n) == oracle.canon(exp["coeffs"])).all()
    assert (region[:pad].reshape(n_ext, polys) == oracle.canon(exp["leaves"])).all()
    assert (region[pad : 2 * pad].reshape(polys, n_ext) == oracle.canon(exp["leaves"]).T).all()
    assert (region[2 * pad : 2 * pad + 4 * nd].reshape(-1, 4) == oracle.canon(exp["digests"])).all()
    assert (region[2 * pad + 4 * nd :].reshape(-1, 4) == oracle.canon(exp["cap"])).all()
    assert (region2[2 * pad :] == region[2 * pad :]).all()


# ---- the whole prover --------------------------------------------------------------------------------------------------

def _lift_circuit(circuit, wires, pis, rng):
    """(circuit with constants, sigmas and k_is lifted, lifted witness, lifted public inputs, number of words lifted)"""
    l_w, c1 = lift(np.asarray(wires, dtype=np.uint64), rng, 1.0)
    l_c, c2 = lift(np.asarray(circuit["constants"], dtype=np.uint64), rng, 1.0)
    l_s, c3 = lift(np.asarray(circuit["sigmas"], dtype=np.uint64), rng, 1.0)
    l_p, c4 = lift(np.asarray(pis, dtype=np.uint64), rng, 1.0)
    l_k = [lift_scalar(k) for k in circuit["k_is"]]
    lifted = dict(circuit, constants=l_c, sigmas=l_s, k_is=l_k, circuit_digest=None)
    return lifted, l_w, l_p, c1 + c2 + c3 + c4 + sum(int(a != b) for a, b in zip(l_k, circuit["k_is"]))


def test_all_25_gates_proof_from_lifted_inputs_equals_the_fixture(gpu):
    """The all-25-gates circuit at 2^14 rows (test_gpu_prove.py::test_all_25_gates_proof_bytes_at_2e14_rows_equal_the_fixture)
    with every liftable word lifted: witness (u32 limbs and bits make half of it liftable), public inputs, constants (the
    selectors are small integers: the gate filter sees s >= p), sigmas and k_is. Circuit digest and proof bytes equal the
    fixture with compiled and with interpreted gates; gl_prove_many with two lifted copies in flight gives the fixture twice."""
    import ed25519_rows as er
    import plonky2_gpu_amd as pg
    from oracle import accel

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    meta = json.load(open(os.path.join(gold, "prove_all_gates_2e14.json")))
    want = open(os.path.join(gold, "prove_all_gates_2e14.bin"), "rb").read()
    assert hashlib.sha256(want).hexdigest() == meta["sha256"]
    with accel.c_backend():
        circuit, wires, pis = er.make_all_gates_circuit(meta["degree_bits"], seed=meta["seed"], templates=meta["templates"],
                                                        fri_params=meta["fri_params"])
    rng = np.random.default_rng(1300)
    lifted, l_w, l_p, count = _lift_circuit(circuit, wires, pis, rng)
    assert count > np.asarray(wires).size // 3
    assert (np.asarray(lifted["constants"])[:6] >= np.uint64(P)).sum() > 1000  # lifted selectors
    for compile_gates in (True, False):
        nc = pg.NativeCircuit(gpu, lifted, compile_gates=compile_gates)
        assert [int(v) for v in nc.circuit_digest] == meta["circuit_digest"], compile_gates
        assert nc.prove_bytes(l_w, l_p) == want, compile_gates
        if compile_gates:
            l_w2, _ = lift(np.asarray(wires, dtype=np.uint64), rng, 0.5)
            other = pg.Context(0)
            try:
                d = [pg.DeviceBuffer.from_host(gpu, np.ascontiguousarray(w)) for w in (l_w, l_w2)]
                assert nc.prove_many(d, [l_p, l_p], [gpu, other]) == [want, want]
                for b in d:
                    b.free()
            finally:
                other.close()
        nc.close()


def test_blinded_proof_from_lifted_inputs(gpu):
    """gl_prove_zk on a small circuit (plonk_instance.make_circuit's, public inputs small enough to be lifted, among them
    2^64 - 1 and 2^64 - 2) with a lifted witness, constants, sigmas and k_is: the canonical witness's bytes. Salts canonical."""
    import plonky2_gpu_amd as pg
    from oracle import prove_ref
    from plonk_instance import make_circuit_instance

    degree_bits, rate_bits, cap_height = 5, 3, 1
    public_inputs = [TOP, TOP2, 12345]
    inst = make_circuit_instance(degree_bits, 23, False, public_inputs=public_inputs)
    cs = prove_ref.commit_from_values(inst["constants"] + inst["sigmas"], rate_bits, cap_height)
    circuit = dict(degree_bits=degree_bits, num_wires=12, num_routed_wires=12, num_constants=inst["num_constants"], num_challenges=2,
                   quotient_degree_factor=8, k_is=inst["k_is"], gates=[("noop", None), ("constant", 2), ("public_input", None), ("arithmetic", 3)],
                   selector_indices=inst["selector_indices"], groups=inst["groups"], num_gate_constraints=4, constants=inst["constants"],
                   sigmas=inst["sigmas"], fri_params=dict(rate_bits=rate_bits, cap_height=cap_height, reduction_arity_bits=[2, 1],
                                                          proof_of_work_bits=3, num_query_rounds=3, hiding=True),
                   circuit_digest=None)
    wires = np.asarray(inst["wires"], dtype=np.uint64)
    rng = np.random.default_rng(1400)
    lifted, l_w, l_p, count = _lift_circuit(circuit, wires, public_inputs, rng)
    assert count > 60 and all(int(x) >= P for x in l_p[:2])
    n_ext = 1 << (degree_bits + rate_bits)
    salts = np.random.default_rng(1401).integers(0, P, size=(3, 4, n_ext), dtype=np.uint64)
    nc = pg.NativeCircuit(gpu, circuit, compile_gates=True)
    want = nc.prove_bytes(wires, public_inputs, salts=salts)
    nc.close()
    parsed = pg.serialization.proof_from_bytes(want, circuit)
    assert prove_ref.verify(dict(circuit, circuit_digest=prove_ref.circuit_digest(cs["cap"], degree_bits), constants_sigmas=cs), parsed)
    nc = pg.NativeCircuit(gpu, lifted, compile_gates=True)
    assert nc.prove_bytes(l_w, l_p, salts=salts) == want
    nc.close()


# ---- STARKs: gl_stark_permutation_zs, gl_stark_quotient_polys, gl_stark_prove ---------------------------------------------------

def _stark_modules():
    import generic_prove_ref as gr
    import stark_fuzz as sf
    import stark_instances as si
    import stark_ref as sr

    return gr, sf, si, sr


def _small_sets(rng, qdf, num_challenges):
    """[set][challenge] (beta, gamma): liftable values, 2^32 - 2 and 2^32 - 3 (lifted: 2^64 - 1, 2^64 - 2) among them"""
    sets = [[(int(rng.integers(0, LIFTABLE)), int(rng.integers(0, LIFTABLE))) for _ in range(num_challenges)] for _ in range(qdf)]
    sets[0][0] = (TOP, TOP2)
    sets[-1][-1] = (sets[-1][-1][0], TOP)
    return sets, [[(lift_scalar(b), lift_scalar(g)) for b, g in s] for s in sets]


def _native_stark(gpu, stark, degree_bits, num_challenges, rate_bits, immediates=None, **fri):
    import plonky2_gpu_amd as pg

    _, _, si, _ = _stark_modules()
    desc = stark.desc(degree_bits, num_challenges, si.fri_params(rate_bits=rate_bits, **fri))
    if immediates is not None:
        desc.immediates = list(immediates)  # as they are: StarkDesc reduces its own
    return pg.NativeStark(gpu, desc)


@pytest.mark.parametrize("name,degree_bits,num_challenges", [("B", 11, 3), ("D17", 3, 4)])
def test_stark_permutation_zs(gpu, name, degree_bits, num_challenges):
    """the trace (any words: the Zs of a trace that satisfies nothing are as well defined), betas and gammas. B at 2^11 rows:
    5 Zs over two blocks of the prefix product each; D(17): 8 instances in one batch, 16 challenge sets"""
    _, _, si, sr = _stark_modules()
    stark = si.STARKS[name]
    rng = np.random.default_rng(1500 + degree_bits)
    n = 1 << degree_bits
    trace = field_data(rng, (stark.num_columns, n))
    l_trace, count = lift(trace, rng, 0.6)
    assert count > trace.size // 4
    sets, l_sets = _small_sets(rng, sr.quotient_degree_factor(stark), num_challenges)
    assert l_sets[0][0] == (M64, M64 - 1)
    ns = _native_stark(gpu, stark, degree_bits, num_challenges, 4)
    try:
        canon_out = ns.permutation_zs(trace, sets)
        _check(ns.permutation_zs(l_trace, l_sets), canon_out)
        _check(ns.permutation_zs(l_trace, l_sets, trace_stride=n + 6), canon_out)
    finally:
        ns.close()
    exp = sr.compute_permutation_z_polys(stark, num_challenges, trace.tolist(), sets)
    assert (canon_out == np.array(exp, dtype=np.uint64)).all()


def _stark_quotient_data(rng, stark, degree_bits, rate_bits, num_challenges, sr):
    n_ext = 1 << (degree_bits + rate_bits)
    trace = field_data(rng, (stark.num_columns, n_ext))
    zs = field_data(rng, (sr.num_zs(stark, num_challenges), n_ext))
    l_trace, c1 = lift(trace, rng, 0.6)
    l_zs, c2 = lift(zs, rng, 0.6)
    assert c1 + c2 > (trace.size + zs.size) // 4
    sets, l_sets = _small_sets(rng, sr.quotient_degree_factor(stark), num_challenges)
    alphas = [TOP, TOP2, int(rng.integers(0, LIFTABLE)), 7][:num_challenges]
    pis = [TOP2, int(rng.integers(0, LIFTABLE)), TOP][: stark.num_public_inputs]
    canon = (trace, zs, sets, alphas, pis)
    lifted = (l_trace, l_zs, l_sets, [lift_scalar(a) for a in alphas], [lift_scalar(x) for x in pis])
    assert all(x >= P for x in lifted[3] + lifted[4])
    return canon, lifted


def _run_quotient(gpu, ns, data, stride=None):
    trace, zs, sets, alphas, pis = data
    d_t = _buf(gpu, trace)
    d_z = _buf(gpu, zs) if zs is not None else None
    return ns.quotient_polys(d_t, d_z, stride or trace.shape[1], alphas, sets, pis)


@pytest.mark.parametrize("name,degree_bits,rate_bits,num_challenges", [("B", 3, 2, 3), ("D17", 2, 4, 4)])
def test_stark_quotient_polys(gpu, name, degree_bits, rate_bits, num_challenges):
    """the trace and Z "LDEs" (any words), alphas, betas, gammas and public inputs lifted; then, through a second handle, the
    immediates of the description lifted as well — ACC weights among B's: gl_stark_create reduces them before it checks the
    ACC contract. SP_ACC adds the 32-bit halves of the raw register: a lifted word x + p has other halves than x"""
    _, sf, si, sr = _stark_modules()
    stark = si.STARKS[name]
    rng = np.random.default_rng(1600 + degree_bits)
    canon, lifted = _stark_quotient_data(rng, stark, degree_bits, rate_bits, num_challenges, sr)
    l_imms = [lift_scalar(v) for v in stark.immediates]
    assert sum(a != b for a, b in zip(l_imms, stark.immediates)) > len(l_imms) // 4
    ns = _native_stark(gpu, stark, degree_bits, num_challenges, rate_bits)
    ns2 = _native_stark(gpu, stark, degree_bits, num_challenges, rate_bits, immediates=l_imms)
    try:
        canon_out = _run_quotient(gpu, ns, canon)
        _check(_run_quotient(gpu, ns, lifted), canon_out)
        _check(_run_quotient(gpu, ns2, canon), canon_out)
        _check(_run_quotient(gpu, ns2, lifted), canon_out)
    finally:
        ns.close()
        ns2.close()
    case = dict(stark=stark, degree_bits=degree_bits, rate_bits=rate_bits, num_challenges=num_challenges)
    assert (canon_out == sf.reference_quotient(case, *canon)).all()


def test_stark_quotient_polys_extreme_accumulators(gpu):
    """every "LDE" word 2^64 - 1 or p - 1 (the data of test_reduce_polys_base's extreme case) under ACC weights 2^31 on one
    accumulator and 2^30 - 1 twice on another: the largest accumulator halves the contract permits with the largest register
    halves a u64 can have. The reference receives the canonical words 2^32 - 2 and p - 1."""
    _, sf, si, sr = _stark_modules()
    from plonky2_gpu_amd.stark import StarkAsm

    a = StarkAsm()
    x, y = a.local(0), a.next(1)
    a.acc(x, 1 << 31, q=2)
    a.acc(x, (1 << 30) - 1, q=1)
    a.acc(y, (1 << 30) - 1, q=1)
    a.emit(a.accr(2))
    a.emit_transition(a.accr(1))
    a.emit_first_row(a.mul(x, y))
    a.emit_last_row(a.sub(x, y))
    a.emit(a.add(x, y))
    instrs, imms = a.program()
    sr.validate_program(instrs, imms, 2, 0)
    stark = sf.FuzzStark(2, 0, 3, [], instrs, imms)
    degree_bits, rate_bits, nch = 4, 2, 2
    case = dict(stark=stark, degree_bits=degree_bits, rate_bits=rate_bits, num_challenges=nch)
    rng = np.random.default_rng(1700)
    pick = rng.random((2, 1 << (degree_bits + rate_bits))) < 0.5
    trace = np.where(pick, np.uint64(TOP), np.uint64(P - 1)).astype(np.uint64)
    l_trace = np.where(pick, np.uint64(M64), np.uint64(P - 1)).astype(np.uint64)
    assert int(pick.sum()) > pick.size // 4
    alphas = [TOP, TOP2]
    import plonky2_gpu_amd as pg

    ns = pg.NativeStark(gpu, pg.stark.StarkDesc(degree_bits, 2, 0, 3, nch, si.fri_params(rate_bits=rate_bits), instrs, imms, []))
    try:
        canon_out = _run_quotient(gpu, ns, (trace, None, None, alphas, []))
        _check(_run_quotient(gpu, ns, (l_trace, None, None, [M64, M64 - 1], [])), canon_out)
    finally:
        ns.close()
    exp = sf.reference_quotient(case, trace, None, None, alphas, [])
    assert exp.any() and (canon_out == exp).all()


def _proof_words(x):
    """every integer of a parsed proof (hashes of the Keccak hasher are bytes: no field words)"""
    if isinstance(x, dict):
        return [w for v in x.values() for w in _proof_words(v)]
    if isinstance(x, (list, tuple)):
        return [w for v in x for w in _proof_words(v)]
    if isinstance(x, (int, np.integer)):
        return [int(x)]
    return []


def test_stark_proof_from_a_lifted_trace(gpu):
    """gl_stark_prove on a valid trace of B (two of its five columns are counters: small values) with nearly every liftable cell
    and both public inputs lifted: the bytes of the canonical trace's proof, which are the reference's; every field word of the
    proof is canonical, the public inputs at its end included"""
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    gr, _, si, sr = _stark_modules()
    degree_bits, nch = 6, 2
    fri = dict(cap_height=1, arity_bits=(2, 1))
    trace, pis = si.B.make_trace(degree_bits, seed=3)
    trace = np.array(trace, dtype=np.uint64)
    rng = np.random.default_rng(1800)
    l_trace, count = lift(trace, rng, 0.95)
    l_pis = [lift_scalar(x) for x in pis]
    assert count > trace.size // 4 and all(x >= P for x in l_pis)
    ns = _native_stark(gpu, si.B, degree_bits, nch, 2, **fri)
    try:
        want = ns.prove_bytes(trace, pis)
        got = ns.prove_bytes(l_trace, l_pis)
    finally:
        ns.close()
    assert got == want
    parsed = pstark.proof_from_bytes(got, ns.desc)
    words = _proof_words(parsed)
    assert len(words) > 500 and all(0 <= w < P for w in words)
    assert [int(x) for x in parsed["public_inputs"]] == [int(x) for x in pis]
    assert got[-16:] == np.array(pis, dtype="<u8").tobytes()
    with accel.c_backend():
        hasher = gr.PoseidonHasher()
        assert want == sr.proof_bytes(hasher, sr.prove(hasher, si.B, nch, si.fri_params(rate_bits=2, **fri), trace.tolist(), pis))
