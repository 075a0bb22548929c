"""starky's prover and verifier restated in pure Python (TEST INFRASTRUCTURE ONLY): the independent reference gl_stark_prove,
gl_stark_permutation_zs and gl_stark_quotient_polys are held against.

    prove                starky/src/prover.rs:32-195 with compute_quotient_polys (:199-319)
    permutation Zs       starky/src/permutation.rs:66-118, 153-179, 229-250; eval_permutation_checks :263-323
    the consumer         starky/src/constraint_consumer.rs:33-77
    verify               starky/src/verifier.rs:42-147 with eval_l_0_and_l_last (:221-235); get_challenges.rs:21-73
    the FRI instance     starky/src/stark.rs:88-137; the openings' order proof.rs:138-182

Hasher-generic like tests/generic_prove_ref.py, whose commits, transcript helpers, prove_openings and verify_fri_proof it uses; the
algebra is oracle/fri_ref.py's and oracle/pyref.py's, looked up as module attributes at call time (oracle.accel.c_backend speeds it up).

A STARK here is an object with num_columns, num_public_inputs, constraint_degree, pairs (lists of (lhs, rhs) columns), instrs /
immediates (the register program, include/plonky2_hip.h) and `closure(F, local, nxt, pis, consumer)`, the same constraints written
by hand: every function that evaluates constraints takes `evaluator`, "program" (the interpreter below) or "closure", and the two
must agree (tests/test_stark_ref.py) so that a wrong program and a wrong interpreter cannot cancel. Constraints are evaluated over
a field object F: Base (the prover's points) or Ext (the verifier's zeta).

Where the device computes in closed form, this file follows the reference's own route: the Lagrange selectors by LDE of the
selector columns (prover.rs:231-235), Z_H(x) as x^n - 1.

The wire format is the one include/plonky2_hip.h defines for StarkProofWithPublicInputs, written here from the header's text."""
import numpy as np

import generic_prove_ref as gr
from oracle import fri_ref, plonk_ref, pyref

P = pyref.P
(LOAD_WIRE, LOAD_CONST, LOAD_PI, LOAD_IMM, ADD, SUB, MUL, EMIT, MULK, ACC, ACCR, LOAD_NEXT, EMIT_TRANSITION, EMIT_FIRST_ROW,
 EMIT_LAST_ROW) = range(15)
MAX_REGS, ACC_LIMIT = 64, 1 << 63


class Base:
    zero, one = 0, 1
    add = staticmethod(lambda x, y: (x + y) % P)
    sub = staticmethod(lambda x, y: (x - y) % P)
    mul = staticmethod(lambda x, y: x * y % P)
    lift = staticmethod(lambda x: int(x) % P)


class Ext:
    zero, one = (0, 0), (1, 0)
    add = staticmethod(fri_ref.ext_add)
    sub = staticmethod(fri_ref.ext_sub)
    mul = staticmethod(fri_ref.ext_mul)
    lift = staticmethod(lambda x: (int(x) % P, 0))


class Consumer:
    """ConstraintConsumer (constraint_consumer.rs:33-77): acc <- acc * alpha + constraint for every alpha, in emission order"""

    def __init__(self, F, alphas, z_last, lagrange_first, lagrange_last):
        self.F, self.alphas = F, [F.lift(a) for a in alphas]
        self.z_last, self.lagrange_first, self.lagrange_last = z_last, lagrange_first, lagrange_last
        self.accs = [F.zero] * len(alphas)
        self.emitted = []  # the constraints as emitted, for the comparison of the two evaluators

    def constraint(self, c):
        self.emitted.append(c)
        self.accs = [self.F.add(self.F.mul(acc, alpha), c) for acc, alpha in zip(self.accs, self.alphas)]

    def constraint_transition(self, c):
        self.constraint(self.F.mul(c, self.z_last))

    def constraint_first_row(self, c):
        self.constraint(self.F.mul(c, self.lagrange_first))

    def constraint_last_row(self, c):
        self.constraint(self.F.mul(c, self.lagrange_last))


# ---------------------------------------------------------------- the register program
def validate_program(instrs, immediates, num_columns, num_public_inputs):
    """What gl_stark_create refuses, restated: raises ValueError"""
    written, bound, used, emitted = set(), [0] * 4, [False] * 4, 0
    for pc, (op, dst, a, b) in enumerate([tuple(int(x) for x in row) for row in instrs]):
        where = "instruction %d: " % pc
        if op == LOAD_CONST:
            raise ValueError(where + "LOAD_CONST in a STARK program")
        if op > EMIT_LAST_ROW:
            raise ValueError(where + "unknown opcode")
        is_emit = op in (EMIT, EMIT_TRANSITION, EMIT_FIRST_ROW, EMIT_LAST_ROW)
        reads = ([a] if op in (ADD, SUB, MUL, MULK, ACC) or is_emit else []) + ([b] if op in (ADD, SUB, MUL) else [])
        if any(r >= MAX_REGS or r not in written for r in reads):
            raise ValueError(where + "register out of range or read before any write")
        if op in (LOAD_WIRE, LOAD_NEXT) and a >= num_columns:
            raise ValueError(where + "column out of range")
        if op == LOAD_PI and a >= num_public_inputs:
            raise ValueError(where + "public input out of range")
        if op == LOAD_IMM and a >= len(immediates):
            raise ValueError(where + "immediate out of range")
        if op == MULK and b >= 64:
            raise ValueError(where + "MULK shift out of range")
        if op == ACC:
            if dst >= 4 or b >= len(immediates) or immediates[b] % P >= 1 << 32:
                raise ValueError(where + "ACC: accumulator or immediate out of range")
            bound[dst] += (immediates[b] % P) * 0xFFFFFFFF
            if bound[dst] >= ACC_LIMIT:
                raise ValueError(where + "ACC: broken overflow contract")
            used[dst] = True
        elif op == ACCR:
            if a >= 4 or not used[a]:
                raise ValueError(where + "ACCR of an empty accumulator")
            bound[a], used[a] = 0, False
        if not is_emit and op != ACC:
            if dst >= MAX_REGS:
                raise ValueError(where + "register out of range")
            written.add(dst)
        emitted += is_emit
    if not emitted:
        raise ValueError("a program with no EMIT")


def run_program(F, instrs, immediates, local, nxt, pis, consumer):
    regs, acc = {}, [F.zero] * 4
    for op, dst, a, b in ([int(x) for x in row] for row in instrs):
        if op == LOAD_WIRE:
            regs[dst] = local[a]
        elif op == LOAD_NEXT:
            regs[dst] = nxt[a]
        elif op == LOAD_PI:
            regs[dst] = pis[a]
        elif op == LOAD_IMM:
            regs[dst] = F.lift(immediates[a])
        elif op == ADD:
            regs[dst] = F.add(regs[a], regs[b])
        elif op == SUB:
            regs[dst] = F.sub(regs[a], regs[b])
        elif op == MUL:
            regs[dst] = F.mul(regs[a], regs[b])
        elif op == MULK:
            regs[dst] = F.mul(regs[a], F.lift(1 << b))
        elif op == ACC:
            acc[dst] = F.add(acc[dst], F.mul(regs[a], F.lift(immediates[b])))
        elif op == ACCR:
            regs[dst], acc[a] = acc[a], F.zero
        elif op == EMIT:
            consumer.constraint(regs[a])
        elif op == EMIT_TRANSITION:
            consumer.constraint_transition(regs[a])
        elif op == EMIT_FIRST_ROW:
            consumer.constraint_first_row(regs[a])
        elif op == EMIT_LAST_ROW:
            consumer.constraint_last_row(regs[a])
        else:
            raise ValueError("opcode %d in a STARK program" % op)


def eval_constraints(F, stark, local, nxt, pis, consumer, evaluator):
    """Stark::eval_packed_generic / eval_ext"""
    if evaluator == "program":
        run_program(F, stark.instrs, stark.immediates, local, nxt, pis, consumer)
    else:
        stark.closure(F, local, nxt, pis, consumer)


# ---------------------------------------------------------------- shape
def quotient_degree_factor(stark):  # stark.rs:79-81
    return max(1, stark.constraint_degree - 1)


def num_zs(stark, num_challenges):  # num_permutation_batches
    return -(-len(stark.pairs) * num_challenges // quotient_degree_factor(stark))


def get_permutation_batches(pairs, challenge_sets, num_challenges, batch_size):
    """permutation.rs:229-250: instance i of a batch takes challenge_sets[i][chal]"""
    instances = [(pair, chal) for pair in pairs for chal in range(num_challenges)]
    return [[(pair, challenge_sets[i][chal]) for i, (pair, chal) in enumerate(instances[k : k + batch_size])]
            for k in range(0, len(instances), batch_size)]


def get_n_permutation_challenge_sets(challenger, num_challenges, num_sets):
    """permutation.rs:153-179: [set][challenge] (beta, gamma)"""
    return [[tuple(challenger.get_n_challenges(2)) for _ in range(num_challenges)] for _ in range(num_sets)]


def compute_permutation_z_polys(stark, num_challenges, trace, challenge_sets):
    """permutation.rs:66-118 -> [num_zs][n] values"""
    n = len(trace[0])
    zs = []
    for instances in get_permutation_batches(stark.pairs, challenge_sets, num_challenges, quotient_degree_factor(stark)):
        z, acc = [], 1
        for r in range(n):
            num = den = 1
            for pair, (beta, gamma) in instances:
                lhs = rhs = gamma
                weight = 1
                for i, j in pair:  # column_pairs.zip(beta.powers())
                    lhs = (lhs + trace[i][r] * weight) % P
                    rhs = (rhs + trace[j][r] * weight) % P
                    weight = weight * beta % P
                num, den = num * lhs % P, den * rhs % P
            z.append(acc)
            acc = acc * num % P * pow(den, P - 2, P) % P
        zs.append(z)
    return zs


def eval_permutation_checks(F, stark, num_challenges, local, local_zs, next_zs, challenge_sets, consumer):
    """permutation.rs:263-323"""
    for z in local_zs:
        consumer.constraint_first_row(F.sub(z, F.one))
    for i, instances in enumerate(get_permutation_batches(stark.pairs, challenge_sets, num_challenges, quotient_degree_factor(stark))):
        prod_l, prod_r = F.one, F.one
        for pair, (beta, gamma) in instances:
            lhs = rhs = F.zero
            for a, b in reversed(pair):  # ReducingFactor::reduce: sum_j beta^j x_j
                lhs = F.add(F.mul(lhs, F.lift(beta)), local[a])
                rhs = F.add(F.mul(rhs, F.lift(beta)), local[b])
            prod_l, prod_r = F.mul(prod_l, F.add(lhs, F.lift(gamma))), F.mul(prod_r, F.add(rhs, F.lift(gamma)))
        consumer.constraint(F.sub(F.mul(next_zs[i], prod_r), F.mul(local_zs[i], prod_l)))


def eval_vanishing_poly(F, stark, num_challenges, local, nxt, pis, perm, consumer, evaluator):
    """vanishing_poly.rs:16-41; perm = (local_zs, next_zs, challenge_sets) or None"""
    eval_constraints(F, stark, local, nxt, pis, consumer, evaluator)
    if perm is not None:
        eval_permutation_checks(F, stark, num_challenges, local, perm[0], perm[1], perm[2], consumer)


# ---------------------------------------------------------------- prove
def _coset_fft(coeffs, size):
    scaled = [c * pow(pyref.GENERATOR, i, P) % P for i, c in enumerate(coeffs)] + [0] * (size - len(coeffs))
    return pyref.fast_ntt(scaled)


def _coset_ifft(values):
    inv = pow(pyref.GENERATOR, P - 2, P)
    return [c * pow(inv, i, P) % P for i, c in enumerate(pyref.fast_ntt(list(values), inverse=True))]


def lde_leaves(values, rate_bits):
    """the leaves of PolynomialBatch::from_values without the tree: row reverse_bits(idx) holds the LDE's values at 7 w^idx"""
    size = len(values[0]) << rate_bits
    lde = [_coset_fft(pyref.fast_ntt(list(v), inverse=True), size) for v in values]
    bits = pyref.log2_strict(size)
    return [[col[pyref.reverse_bits(i, bits)] for col in lde] for i in range(size)]


def compute_quotient_polys(stark, num_challenges, degree_bits, rate_bits, trace_leaves, zs_leaves, challenge_sets, pis, alphas,
                           evaluator="program"):
    """prover.rs:199-319 -> [num_challenges][n << qdb] coefficients. `trace_leaves` / `zs_leaves`: the commitments' leaves (row
    reverse_bits(idx) of the LDE), zs_leaves None without pairs"""
    n = 1 << degree_bits
    qdb = (quotient_degree_factor(stark) - 1).bit_length()
    assert qdb <= rate_bits, "Having constraints of degree higher than the rate is not supported yet."
    step, next_step, size, bits = 1 << (rate_bits - qdb), 1 << qdb, n << qdb, degree_bits + rate_bits
    selector = lambda k: pyref.fast_ntt([1 if i == k else 0 for i in range(n)], inverse=True)  # noqa: E731
    lagrange_first, lagrange_last = _coset_fft(selector(0), size), _coset_fft(selector(n - 1), size)
    last = pow(pyref.root_of_unity(degree_bits), P - 2, P)
    w = pyref.root_of_unity(degree_bits + qdb)
    pis = [int(p) % P for p in pis]
    values = [[] for _ in range(num_challenges)]
    x = pyref.GENERATOR
    for i in range(size):
        row, row_next = pyref.reverse_bits(i * step, bits), pyref.reverse_bits(((i + next_step) % size) * step, bits)
        consumer = Consumer(Base, alphas, (x - last) % P, lagrange_first[i], lagrange_last[i])
        perm = None if zs_leaves is None else (zs_leaves[row], zs_leaves[row_next], challenge_sets)
        eval_vanishing_poly(Base, stark, num_challenges, trace_leaves[row], trace_leaves[row_next], pis, perm, consumer, evaluator)
        z_h_inv = pow((pow(x, n, P) - 1) % P, P - 2, P)
        for k, acc in enumerate(consumer.accs):
            values[k].append(acc * z_h_inv % P)
        x = x * w % P
    return [_coset_ifft(v) for v in values]


def fri_instance(stark, num_challenges, zeta, degree_bits):
    """stark.rs:88-137: oracles trace, [Zs], quotient; everything at zeta, then trace and Zs at g * zeta"""
    sizes = [stark.num_columns] + ([num_zs(stark, num_challenges)] if stark.pairs else []) + [quotient_degree_factor(stark) * num_challenges]
    infos = [[(oi, pi) for pi in range(k)] for oi, k in enumerate(sizes)]
    g_zeta = fri_ref.ext_mul((pyref.root_of_unity(degree_bits), 0), zeta)
    return dict(batches=[(zeta, [p for info in infos for p in info]), (g_zeta, [p for info in infos[:-1] for p in info])])


def to_fri_openings(op):
    """proof.rs:161-182"""
    return [op["local_values"] + (op["permutation_zs"] or []) + op["quotient_polys"], op["next_values"] + (op["permutation_zs_next"] or [])]


def prove(hasher, stark, num_challenges, fri_params, trace, public_inputs, evaluator="program"):
    """prover.rs:32-195; `trace` [num_columns][n] values"""
    rate_bits, cap_height = fri_params["rate_bits"], fri_params["cap_height"]
    assert not fri_params.get("hiding")
    n = len(trace[0])
    degree_bits = pyref.log2_strict(n)
    assert sum(fri_params["reduction_arity_bits"]) <= degree_bits + rate_bits - cap_height, "FRI total reduction arity is too large."
    qdf = quotient_degree_factor(stark)
    trace_c = gr.commit_from_values(hasher, trace, rate_bits, cap_height)
    ch = fri_ref.Challenger()
    gr.observe_cap(hasher, ch, trace_c["cap"])
    zs_c = challenge_sets = None
    if stark.pairs:
        challenge_sets = get_n_permutation_challenge_sets(ch, num_challenges, qdf)
        zs_c = gr.commit_from_values(hasher, compute_permutation_z_polys(stark, num_challenges, trace, challenge_sets), rate_bits, cap_height)
        gr.observe_cap(hasher, ch, zs_c["cap"])
    alphas = ch.get_n_challenges(num_challenges)
    quotient_polys = compute_quotient_polys(stark, num_challenges, degree_bits, rate_bits, trace_c["leaves"], zs_c and zs_c["leaves"],
                                            challenge_sets, public_inputs, alphas, evaluator)
    chunks = []
    for q in quotient_polys:
        assert all(c == 0 for c in q[n * qdf :]), "Quotient has failed, the vanishing polynomial is not divisible by Z_H"
        chunks += [q[k : k + n] for k in range(0, n * qdf, n)]
    quot_c = gr.commit_from_coeffs(hasher, chunks, rate_bits, cap_height)
    gr.observe_cap(hasher, ch, quot_c["cap"])
    zeta = ch.get_extension_challenge()
    assert fri_ref.ext_pow(zeta, n) != (1, 0), "Opening point is in the subgroup."
    g_zeta = fri_ref.ext_mul((pyref.root_of_unity(degree_bits), 0), zeta)
    ev = lambda c, z: [plonk_ref.eval_ext2(p, z) for p in c["polynomials"]]  # noqa: E731
    openings = dict(local_values=ev(trace_c, zeta), next_values=ev(trace_c, g_zeta), permutation_zs=zs_c and ev(zs_c, zeta),
                    permutation_zs_next=zs_c and ev(zs_c, g_zeta), quotient_polys=ev(quot_c, zeta))
    for batch in to_fri_openings(openings):
        ch.observe_extension_elements(batch)
    oracles = [trace_c] + ([zs_c] if zs_c else []) + [quot_c]
    opening_proof = gr.prove_openings(hasher, fri_instance(stark, num_challenges, zeta, degree_bits), oracles, ch, fri_params)
    return dict(trace_cap=trace_c["cap"], permutation_zs_cap=zs_c and zs_c["cap"], quotient_polys_cap=quot_c["cap"], openings=openings,
                opening_proof=opening_proof, public_inputs=[int(p) % P for p in public_inputs])


# ---------------------------------------------------------------- verify
def get_challenges(hasher, stark, num_challenges, fri_params, proof, degree_bits):
    """get_challenges.rs:21-73"""
    ch = fri_ref.Challenger()
    gr.observe_cap(hasher, ch, proof["trace_cap"])
    challenge_sets = None
    if proof["permutation_zs_cap"] is not None:
        challenge_sets = get_n_permutation_challenge_sets(ch, num_challenges, quotient_degree_factor(stark))
        gr.observe_cap(hasher, ch, proof["permutation_zs_cap"])
    alphas = ch.get_n_challenges(num_challenges)
    gr.observe_cap(hasher, ch, proof["quotient_polys_cap"])
    zeta = ch.get_extension_challenge()
    for batch in to_fri_openings(proof["openings"]):
        ch.observe_extension_elements(batch)
    return dict(permutation_challenge_sets=challenge_sets, stark_alphas=alphas, stark_zeta=zeta,
                fri_challenges=gr.fri_challenges(hasher, ch, proof["opening_proof"], degree_bits, fri_params))


def eval_l_0_and_l_last(log_n, x):
    """verifier.rs:221-235 over the extension: L_0 = (x^n - 1) / (n (x - 1)), L_last = (x^n - 1) / (n (g x - 1))"""
    n, g = (1 << log_n, 0), (pyref.root_of_unity(log_n), 0)
    z_x = fri_ref.ext_sub(fri_ref.ext_pow(x, 1 << log_n), (1, 0))
    inv = lambda d: fri_ref.ext_mul(z_x, fri_ref.ext_inv(fri_ref.ext_mul(n, d)))  # noqa: E731
    return inv(fri_ref.ext_sub(x, (1, 0))), inv(fri_ref.ext_sub(fri_ref.ext_mul(g, x), (1, 0)))


def verify(hasher, stark, num_challenges, fri_params, proof, evaluator="program"):
    """verify_stark_proof (verifier.rs:19-147). Returns True or raises AssertionError."""
    op = proof["openings"]
    perm = bool(stark.pairs)
    # validate_proof_shape (:149-219)
    assert len(proof["public_inputs"]) == stark.num_public_inputs
    lde_bits = fri_params["cap_height"] + len(proof["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"][0][1])
    degree_bits = lde_bits - fri_params["rate_bits"]  # recover_degree_bits
    qdf = quotient_degree_factor(stark)
    assert len(proof["trace_cap"]) == len(proof["quotient_polys_cap"]) == 1 << fri_params["cap_height"]
    assert len(op["local_values"]) == len(op["next_values"]) == stark.num_columns and len(op["quotient_polys"]) == qdf * num_challenges
    if perm:
        assert proof["permutation_zs_cap"] is not None and len(proof["permutation_zs_cap"]) == 1 << fri_params["cap_height"]
        assert len(op["permutation_zs"]) == len(op["permutation_zs_next"]) == num_zs(stark, num_challenges)
    else:
        assert proof["permutation_zs_cap"] is None and op["permutation_zs"] is None and op["permutation_zs_next"] is None
    chal = get_challenges(hasher, stark, num_challenges, fri_params, proof, degree_bits)
    zeta = chal["stark_zeta"]
    l_0, l_last = eval_l_0_and_l_last(degree_bits, zeta)
    last = pow(pyref.root_of_unity(degree_bits), P - 2, P)
    consumer = Consumer(Ext, chal["stark_alphas"], fri_ref.ext_sub(zeta, (last, 0)), l_0, l_last)
    perm_data = (op["permutation_zs"], op["permutation_zs_next"], chal["permutation_challenge_sets"]) if perm else None
    eval_vanishing_poly(Ext, stark, num_challenges, op["local_values"], op["next_values"], [Ext.lift(p) for p in proof["public_inputs"]], perm_data,
                        consumer, evaluator)
    zeta_pow_deg = fri_ref.ext_pow(zeta, 1 << degree_bits)
    z_h_zeta = fri_ref.ext_sub(zeta_pow_deg, (1, 0))
    for i in range(num_challenges):
        t = fri_ref.reduce_with_powers_ext(op["quotient_polys"][i * qdf : (i + 1) * qdf], zeta_pow_deg)
        assert tuple(consumer.accs[i]) == tuple(fri_ref.ext_mul(z_h_zeta, t)), "Mismatch between evaluation and opening of quotient polynomial"
    caps = [proof["trace_cap"]] + ([proof["permutation_zs_cap"]] if perm else []) + [proof["quotient_polys_cap"]]
    return gr.verify_fri_proof(hasher, fri_instance(stark, num_challenges, zeta, degree_bits), to_fri_openings(op), chal["fri_challenges"], caps,
                               proof["opening_proof"], degree_bits, fri_params)


# ---------------------------------------------------------------- wire format (include/plonky2_hip.h, gl_stark_prove)
def _u64(xs):
    return np.array([int(x) % P for x in xs], dtype="<u8").tobytes()


def _flat_ext(v):
    return [c for e in v for c in e]


def proof_bytes(hasher, proof):
    hashes = lambda hs: b"".join(hasher.to_bytes(h) for h in hs)  # noqa: E731
    out = [hashes(proof["trace_cap"])]
    if proof["permutation_zs_cap"] is not None:
        out.append(hashes(proof["permutation_zs_cap"]))
    out.append(hashes(proof["quotient_polys_cap"]))
    op = proof["openings"]
    for k in ("local_values", "next_values", "permutation_zs", "permutation_zs_next", "quotient_polys"):
        if op[k] is not None:
            out.append(_u64(_flat_ext(op[k])))
    fp = proof["opening_proof"]  # write_fri_proof (util/serialization.rs)
    out += [hashes(cap) for cap in fp["commit_phase_merkle_caps"]]
    for rnd in fp["query_round_proofs"]:
        for evals, sib in rnd["initial_trees_proof"]:
            out += [_u64(evals), bytes([len(sib)]), hashes(sib)]
        for st in rnd["steps"]:
            out += [_u64(_flat_ext(st["evals"])), bytes([len(st["merkle_proof"])]), hashes(st["merkle_proof"])]
    out += [_u64(_flat_ext(fp["final_poly"])), _u64([fp["pow_witness"]]), _u64(proof["public_inputs"])]
    return b"".join(out)
