"""prove() and verify() with the Merkle hasher as a parameter (TEST INFRASTRUCTURE ONLY): the independent prover the
KeccakGoldilocksConfig proofs of the library are held against (plonky2/src/plonk/config.rs:110-128: Hasher = PoseidonHash or
KeccakHash<25>, InnerHasher = PoseidonHash either way).

Restated here is exactly what depends on C::Hasher: the commitment's tree, the circuit digest (plonk/circuit_builder.rs:915-927),
observe_hash / observe_cap (iop/challenger.rs:66-85: the elements of GenericHashOut::to_vec), the FRI commit-phase trees,
MerkleTree::prove and verify_merkle_proof_to_cap, the verifier's Merkle checks and the wire format of a hash
(util/serialization.rs:537-543). Everything else — the permutation argument, gate constraints, quotient, openings, the FRI algebra,
the Challenger's sponge, proof of work — is oracle/'s, taken as it is and looked up as MODULE ATTRIBUTES at call time, so that
`with oracle.accel.c_backend():` speeds this prover up like the oracle's own.

A hasher object has HASH_SIZE, hash_no_pad, hash_pad, hash_or_noop, two_to_one, to_vec, to_bytes (the reference's Hasher and
GenericHashOut traits) and, because a tree layer is hashed at once, hash_or_noop_batch and two_to_one_batch. A hash is an opaque
value with ==: a list of four ints (PoseidonHasher) or `bytes` of length 25 (KeccakHasher).

Pins (tests/test_generic_prove_ref.py): with PoseidonHasher the proof dict and bytes of oracle/prove_ref.py + serialize_ref.py; with
KeccakHasher prove -> verify and the rejection of tampered proofs, the way the reference pins its own prover; to_vec on vectors
written out by hand."""
import numpy as np

import keccak_ref
from oracle import fri_ref, plonk_ref, prove_ref, pyref

P = pyref.P
SALT_SIZE = 4  # fri/oracle.rs:41


def _hash_pad_input(inputs):
    """Hasher::hash_pad (plonk/config.rs:44-52): pad10*1 up to a multiple of SPONGE_WIDTH = 12"""
    padded = list(inputs) + [1]
    while (len(padded) + 1) % 12 != 0:
        padded.append(0)
    return padded + [1]


class PoseidonHasher:
    """PoseidonHash (hash/poseidon.rs): everything delegates to oracle/pyref.py; a hash is HashOut's four elements"""

    HASH_SIZE = 32
    name = "poseidon"

    def hash_no_pad(self, inputs):
        return pyref.hash_no_pad(list(inputs))

    def hash_pad(self, inputs):
        return self.hash_no_pad(_hash_pad_input(inputs))

    def hash_or_noop(self, inputs):
        return pyref.hash_or_noop(list(inputs))

    def two_to_one(self, left, right):
        return pyref.two_to_one(left, right)

    def hash_or_noop_batch(self, leaves):
        return [self.hash_or_noop(leaf) for leaf in leaves]

    def two_to_one_batch(self, lefts, rights):
        return [self.two_to_one(a, b) for a, b in zip(lefts, rights)]

    def to_vec(self, h):  # HashOut::to_vec (hash/hash_types.rs:96-98)
        return [int(x) % P for x in h]

    def to_bytes(self, h):  # HashOut::to_bytes (:80-86): four canonical little-endian u64
        return np.array([int(x) % P for x in h], dtype="<u8").tobytes()

    def from_bytes(self, b):
        return [int(x) for x in np.frombuffer(b, dtype="<u8")]


class KeccakHasher:
    """KeccakHash<25> (hash/keccak.rs:53-83) on tests/keccak_ref.py; a hash is BytesHash<25>: `bytes` of length 25"""

    HASH_SIZE = 25
    name = "keccak"

    @staticmethod
    def _rows(hashes):
        return [bytes(row) for row in np.asarray(hashes, dtype=np.uint8).reshape(-1, 25)]

    def hash_no_pad(self, inputs):
        return self._rows(keccak_ref.hash_no_pad(np.array([int(x) % P for x in inputs], dtype=np.uint64).reshape(1, -1)))[0]

    def hash_pad(self, inputs):
        return self.hash_no_pad(_hash_pad_input(inputs))

    def hash_or_noop(self, inputs):
        return self.hash_or_noop_batch([inputs])[0]

    def two_to_one(self, left, right):
        return self.two_to_one_batch([left], [right])[0]

    def hash_or_noop_batch(self, leaves):
        """every leaf of a tree at once (they have one length); raises ValueError for 4 elements, where the reference panics"""
        return self._rows(keccak_ref.hash_or_noop(np.array([[int(x) % P for x in leaf] for leaf in leaves], dtype=np.uint64)))

    def two_to_one_batch(self, lefts, rights):
        as_rows = lambda hs: np.frombuffer(b"".join(hs), dtype=np.uint8).reshape(-1, 25)  # noqa: E731
        return self._rows(keccak_ref.two_to_one(as_rows(lefts), as_rows(rights)))

    def to_vec(self, h):
        """BytesHash<25>::to_vec (hash/hash_types.rs:179-189): chunks of 7 bytes (7, 7, 7, 4), each little endian, zero extended"""
        h = bytes(h)
        assert len(h) == 25
        return [int.from_bytes(h[k : k + 7], "little") for k in range(0, 25, 7)]

    def to_bytes(self, h):
        assert len(h) == 25
        return bytes(h)

    def from_bytes(self, b):
        return bytes(b)


# ---------------------------------------------------------------- trees
def merkle_tree(hasher, leaves, cap_height):
    """MerkleTree::new (hash/merkle_tree.rs:283-319) -> (digests, cap), digests in the reference's layout: inside a cap subtree node
    idx of layer L sits at 2 * (((idx >> 1) << (L + 1)) + 2^L - 1) + (idx & 1) (merkle_tree.rs:46-54, 424-435)"""
    n = len(leaves)
    lg = pyref.log2_strict(n)
    assert cap_height <= lg
    n_cap, sub_leaves = 1 << cap_height, n >> cap_height
    sub_digests = 2 * (sub_leaves - 1)
    digests = [None] * (n_cap * sub_digests)
    layer, per_sub, L = hasher.hash_or_noop_batch(leaves), sub_leaves, 0
    while per_sub > 1:
        for g, d in enumerate(layer):
            c, idx = divmod(g, per_sub)
            digests[c * sub_digests + 2 * (((idx >> 1) << (L + 1)) + (1 << L) - 1) + (idx & 1)] = d
        layer = hasher.two_to_one_batch(layer[0::2], layer[1::2])
        per_sub >>= 1
        L += 1
    assert all(d is not None for d in digests) and len(layer) == n_cap
    return digests, layer


def merkle_prove(digests, n_leaves, cap_height, leaf_index):
    """MerkleTree::prove (hash/merkle_tree.rs:392-440)"""
    num_layers = (n_leaves.bit_length() - 1) - cap_height
    tree_len = len(digests) >> cap_height
    base = tree_len * (leaf_index >> num_layers)
    pair_index = leaf_index & ((1 << num_layers) - 1)
    siblings = []
    for i in range(num_layers):
        parity = pair_index & 1
        pair_index >>= 1
        siblings.append(digests[base + 2 * ((pair_index << (i + 1)) + (1 << i) - 1) + (1 - parity)])
    return siblings


def merkle_verify(hasher, leaf, index, cap, siblings):
    """verify_merkle_proof_to_cap (hash/merkle_proofs.rs:53-86)"""
    cur = hasher.hash_or_noop(leaf)
    for s in siblings:
        cur = hasher.two_to_one(s, cur) if index & 1 else hasher.two_to_one(cur, s)
        index >>= 1
    return index < len(cap) and cur == cap[index]


def commit_from_coeffs(hasher, coeffs, rate_bits, cap_height, salt=None):
    """PolynomialBatch::from_coeffs (fri/oracle.rs:911-977); `salt`: SALT_SIZE columns in leaf order (oracle/prove_ref.py)"""
    n_ext = len(coeffs[0]) << rate_bits
    lde = []
    for c in coeffs:
        scaled = [x * pow(pyref.GENERATOR, i, P) % P for i, x in enumerate(c)] + [0] * (n_ext - len(c))
        lde.append(pyref.fast_ntt(scaled))
    lg = pyref.log2_strict(n_ext)
    rev = [pyref.reverse_bits(i, lg) for i in range(n_ext)]
    leaves = [[col[r] for col in lde] for r in rev]
    if salt is not None:
        assert len(salt) == SALT_SIZE and all(len(col) == n_ext for col in salt)
        leaves = [row + [int(col[i]) % P for col in salt] for i, row in enumerate(leaves)]
    digests, cap = merkle_tree(hasher, leaves, cap_height)
    return dict(polynomials=[list(c) for c in coeffs], leaves=leaves, digests=digests, cap=cap)


def commit_from_values(hasher, values, rate_bits, cap_height, salt=None):
    """PolynomialBatch::from_values (fri/oracle.rs:709-731)"""
    return commit_from_coeffs(hasher, [pyref.fast_ntt(list(v), inverse=True) for v in values], rate_bits, cap_height, salt)


# ---------------------------------------------------------------- transcript
def circuit_digest(hasher, constants_sigmas_cap, degree_bits, domain_separator=()):
    """circuit_builder.rs:915-927: hash_no_pad(cap.flatten() || hash_pad(domain separator).to_vec() || [degree_bits])"""
    parts = [x for h in constants_sigmas_cap for x in hasher.to_vec(h)] + hasher.to_vec(hasher.hash_pad(domain_separator)) + [degree_bits]
    return hasher.hash_no_pad(parts)


def observe_hash(hasher, challenger, h):
    """Challenger::observe_hash::<OH> (iop/challenger.rs:66-68)"""
    challenger.observe_elements(hasher.to_vec(h))


def observe_cap(hasher, challenger, cap):
    """Challenger::observe_cap::<OH> (iop/challenger.rs:81-85)"""
    for h in cap:
        observe_hash(hasher, challenger, h)


def with_hasher(hasher, circuit):
    """the circuit dict of tests/plonk_instance.py as the builder of a config with `hasher` would make it: the preprocessed
    commitment and the circuit digest recomputed (circuit_builder.rs:861-873, 915-927)"""
    fp = circuit["fri_params"]
    cs = commit_from_values(hasher, circuit["constants"] + circuit["sigmas"], fp["rate_bits"], fp["cap_height"])
    return dict(circuit, constants_sigmas=cs, circuit_digest=circuit_digest(hasher, cs["cap"], circuit["degree_bits"]))


# ---------------------------------------------------------------- FRI prover
def fri_committed_trees(hasher, coeffs, values, challenger, params):
    """fri/prover.rs:77-120"""
    trees = []
    shift = pyref.GENERATOR
    for arity_bits in params["reduction_arity_bits"]:
        arity = 1 << arity_bits
        values = fri_ref.reverse_index_bits(values)
        leaves = [fri_ref.flatten(values[k : k + arity]) for k in range(0, len(values), arity)]
        digests, cap = merkle_tree(hasher, leaves, params["cap_height"])
        observe_cap(hasher, challenger, cap)
        trees.append(dict(leaves=leaves, digests=digests, cap=cap))
        beta = challenger.get_extension_challenge()
        coeffs = [fri_ref.reduce_with_powers_ext(coeffs[k : k + arity], beta) for k in range(0, len(coeffs), arity)]
        shift = pow(shift, arity, P)
        values = fri_ref.ext_coset_fft(coeffs, shift)
    coeffs = coeffs[: len(coeffs) >> params["rate_bits"]]
    challenger.observe_extension_elements(coeffs)
    return trees, coeffs


def fri_prover_query_rounds(initial_trees, trees, challenger, n, params):
    """fri/prover.rs:173-260"""
    rounds = []
    for rand in challenger.get_n_challenges(params["num_query_rounds"]):
        x_index = rand % n
        initial = [(list(t["leaves"][x_index]), merkle_prove(t["digests"], len(t["leaves"]), params["cap_height"], x_index)) for t in initial_trees]
        steps = []
        for i, t in enumerate(trees):
            ab = params["reduction_arity_bits"][i]
            leaf = t["leaves"][x_index >> ab]
            evals = [(leaf[2 * k], leaf[2 * k + 1]) for k in range(len(leaf) // 2)]
            steps.append(dict(evals=evals, merkle_proof=merkle_prove(t["digests"], len(t["leaves"]), params["cap_height"], x_index >> ab)))
            x_index >>= ab
        rounds.append(dict(initial_trees_proof=initial, steps=steps))
    return rounds


def prove_openings(hasher, instance, oracles, challenger, params):
    """PolynomialBatch::prove_openings (fri/oracle.rs:1047-1112) + fri_proof (fri/prover.rs:24-70)"""
    ext_mul, ext_add = fri_ref.ext_mul, fri_ref.ext_add
    alpha = challenger.get_extension_challenge()
    final_poly = []
    for point, polys in instance["batches"]:
        comp = fri_ref.reduce_polys_base([oracles[oi]["polynomials"][pi] for oi, pi in polys], alpha)
        quotient = fri_ref.divide_by_linear(comp, point)
        scale = fri_ref.ext_pow(alpha, len(polys))
        final_poly = [ext_mul(c, scale) for c in final_poly]
        final_poly = [ext_add(a, b) for a, b in zip(final_poly + [(0, 0)] * (len(quotient) - len(final_poly)), quotient)]
    final_poly = [(0, 0)] + final_poly
    n_lde = len(final_poly) << params["rate_bits"]
    lde_coeffs = final_poly + [(0, 0)] * (n_lde - len(final_poly))
    lde_values = fri_ref.ext_coset_fft(lde_coeffs, pyref.GENERATOR)
    trees, final_coeffs = fri_committed_trees(hasher, lde_coeffs, lde_values, challenger, params)
    pow_witness = fri_ref.fri_proof_of_work(challenger, params)
    rounds = fri_prover_query_rounds(oracles, trees, challenger, n_lde, params)
    return dict(commit_phase_merkle_caps=[t["cap"] for t in trees], query_round_proofs=rounds, final_poly=final_coeffs, pow_witness=pow_witness)


# ---------------------------------------------------------------- prove
def prove(hasher, circuit, wires, public_inputs, salts=None):
    """plonk/prover.rs:40-233 from the full witness on; `circuit` as with_hasher(hasher, ..) gives it; `salts` as in
    oracle/prove_ref.py ([3][SALT_SIZE][n_ext] in leaf order, given exactly when fri_params["hiding"])"""
    fp = circuit["fri_params"]
    hiding = bool(fp.get("hiding"))
    assert hiding == (salts is not None), "salts are given exactly when the circuit is hiding"
    salt_w, salt_z, salt_q = salts if hiding else (None, None, None)
    rate_bits, cap_height = fp["rate_bits"], fp["cap_height"]
    db, n = circuit["degree_bits"], 1 << circuit["degree_bits"]
    nch, qdf, num_routed = circuit["num_challenges"], circuit["quotient_degree_factor"], circuit["num_routed_wires"]
    pih = pyref.hash_no_pad(public_inputs)  # InnerHasher (prover.rs:52)
    wires_c = commit_from_values(hasher, wires, rate_bits, cap_height, salt_w)
    ch = fri_ref.Challenger()
    observe_hash(hasher, ch, circuit["circuit_digest"])
    ch.observe_elements(pih)  # observe_hash::<InnerHasher>
    observe_cap(hasher, ch, wires_c["cap"])
    betas, gammas = ch.get_n_challenges(nch), ch.get_n_challenges(nch)
    assert qdf < num_routed
    subgroup = [pow(pyref.root_of_unity(db), i, P) for i in range(n)]
    zs_pp = plonk_ref.zs_partial_products(wires, circuit["sigmas"], circuit["k_is"], betas, gammas, qdf, subgroup)
    zs_c = commit_from_values(hasher, zs_pp, rate_bits, cap_height, salt_z)
    observe_cap(hasher, ch, zs_c["cap"])
    alphas = ch.get_n_challenges(nch)
    cs = circuit["constants_sigmas"]
    qdb = (qdf - 1).bit_length()
    bits, step = db + rate_bits, 1 << (rate_bits - qdb)
    gates = prove_ref.base_gates(circuit)
    gate_terms = []
    for i in range(n << qdb):
        row = pyref.reverse_bits(i * step, bits)
        gate_terms.append(plonk_ref.evaluate_gate_constraints(gates, circuit["selector_indices"], circuit["groups"], circuit["num_gate_constraints"],
                                                              cs["leaves"][row][: circuit["num_constants"]], wires_c["leaves"][row], pih))
    unsalted = lambda c: [row[: len(c["polynomials"])] for row in c["leaves"]] if hiding else c["leaves"]  # noqa: E731
    quotient_polys = plonk_ref.compute_quotient_polys(unsalted(wires_c), cs["leaves"], unsalted(zs_c), circuit["num_constants"], circuit["k_is"],
                                                      betas, gammas, alphas, db, rate_bits, qdf, gate_terms)
    chunks = []
    for q in quotient_polys:
        assert all(c == 0 for c in q[n * qdf :]), "Quotient has failed, the vanishing polynomial is not divisible by Z_H"
        chunks += [q[k : k + n] for k in range(0, n * qdf, n)]
    quot_c = commit_from_coeffs(hasher, chunks, rate_bits, cap_height, salt_q)
    observe_cap(hasher, ch, quot_c["cap"])
    zeta = ch.get_extension_challenge()
    assert fri_ref.ext_pow(zeta, n) != (1, 0), "Opening point is in the subgroup."
    g_zeta = fri_ref.ext_mul((pyref.root_of_unity(db), 0), zeta)
    ev = lambda c, z: [plonk_ref.eval_ext2(p, z) for p in c["polynomials"]]  # noqa: E731
    cs_eval, zs_eval = ev(cs, zeta), ev(zs_c, zeta)
    openings = dict(constants=cs_eval[: circuit["num_constants"]], plonk_sigmas=cs_eval[circuit["num_constants"] :], wires=ev(wires_c, zeta),
                    plonk_zs=zs_eval[:nch], plonk_zs_next=ev(zs_c, g_zeta)[:nch], partial_products=zs_eval[nch:], quotient_polys=ev(quot_c, zeta))
    for batch in prove_ref.fri_openings(openings):
        ch.observe_extension_elements(batch)
    opening_proof = prove_openings(hasher, prove_ref.fri_instance(circuit, zeta), [cs, wires_c, zs_c, quot_c], ch, fp)
    return dict(wires_cap=wires_c["cap"], plonk_zs_partial_products_cap=zs_c["cap"], quotient_polys_cap=quot_c["cap"], openings=openings,
                opening_proof=opening_proof, public_inputs=list(public_inputs))


# ---------------------------------------------------------------- verify
def fri_challenges(hasher, challenger, proof, degree_bits, params):
    """Challenger::fri_challenges (fri/challenges.rs:24-66)"""
    lde_size = 1 << (degree_bits + params["rate_bits"])
    alpha = challenger.get_extension_challenge()
    betas = []
    for cap in proof["commit_phase_merkle_caps"]:
        observe_cap(hasher, challenger, cap)
        betas.append(challenger.get_extension_challenge())
    challenger.observe_extension_elements(proof["final_poly"])
    challenger.observe_element(proof["pow_witness"])
    pow_response = challenger.get_challenge()
    indices = [challenger.get_challenge() % lde_size for _ in range(params["num_query_rounds"])]
    return dict(fri_alpha=alpha, fri_betas=betas, fri_pow_response=pow_response, fri_query_indices=indices)


def get_challenges(hasher, circuit, proof, pih):
    """plonk/get_challenges.rs:28-75"""
    nch = circuit["num_challenges"]
    ch = fri_ref.Challenger()
    observe_hash(hasher, ch, circuit["circuit_digest"])
    ch.observe_elements(pih)
    observe_cap(hasher, ch, proof["wires_cap"])
    betas, gammas = ch.get_n_challenges(nch), ch.get_n_challenges(nch)
    observe_cap(hasher, ch, proof["plonk_zs_partial_products_cap"])
    alphas = ch.get_n_challenges(nch)
    observe_cap(hasher, ch, proof["quotient_polys_cap"])
    zeta = ch.get_extension_challenge()
    for batch in prove_ref.fri_openings(proof["openings"]):
        ch.observe_extension_elements(batch)
    fri = fri_challenges(hasher, ch, proof["opening_proof"], circuit["degree_bits"], circuit["fri_params"])
    return dict(plonk_betas=betas, plonk_gammas=gammas, plonk_alphas=alphas, plonk_zeta=zeta, fri_challenges=fri)


def verify_fri_proof(hasher, instance, openings, challenges, initial_caps, proof, degree_bits, params):
    """verify_fri_proof (fri/verifier.rs:63-113) with fri_verifier_query_round (:177-258) and fri_combine_initial (:127-175): the
    structure of oracle/fri_ref.py's, its algebra called as it is, the Merkle checks through `hasher`"""
    ext_mul, ext_add, ext_sub, ext_pow, ext_inv = fri_ref.ext_mul, fri_ref.ext_add, fri_ref.ext_sub, fri_ref.ext_pow, fri_ref.ext_inv
    log_n = degree_bits + params["rate_bits"]
    min_lz = params["proof_of_work_bits"] + (64 - P.bit_length())
    assert 64 - challenges["fri_pow_response"].bit_length() >= min_lz, "Invalid proof of work witness."
    assert len(proof["query_round_proofs"]) == params["num_query_rounds"]
    alpha = challenges["fri_alpha"]
    reduced_openings = [fri_ref.reduce_with_powers_ext(vals, alpha) for vals in openings]
    for x_index, rp in zip(challenges["fri_query_indices"], proof["query_round_proofs"]):
        for (evals, mp), cap in zip(rp["initial_trees_proof"], initial_caps):
            assert merkle_verify(hasher, evals, x_index, cap, mp), "initial Merkle proof"
        subgroup_x = pyref.GENERATOR * pow(pyref.root_of_unity(log_n), pyref.reverse_bits(x_index, log_n), P) % P
        s = (0, 0)
        for (point, polys), red_open in zip(instance["batches"], reduced_openings):
            # unsalted_eval (fri/proof.rs:45-52): the salt sits behind the polynomials' values, which the indices never reach
            evals = [(rp["initial_trees_proof"][oi][0][pi], 0) for oi, pi in polys]
            numerator = ext_sub(fri_ref.reduce_with_powers_ext(evals, alpha), red_open)
            denominator = ext_sub((subgroup_x, 0), point)
            s = ext_mul(s, ext_pow(alpha, len(polys)))
            s = ext_add(s, ext_mul(numerator, ext_inv(denominator)))
        old_eval = ext_mul(s, (subgroup_x, 0))
        xi = x_index
        for i, ab in enumerate(params["reduction_arity_bits"]):
            arity = 1 << ab
            evals = rp["steps"][i]["evals"]
            coset_index, within = xi >> ab, xi & (arity - 1)
            assert tuple(evals[within]) == tuple(old_eval), "FRI consistency"
            old_eval = fri_ref.compute_evaluation(subgroup_x, within, ab, evals, challenges["fri_betas"][i])
            assert merkle_verify(hasher, fri_ref.flatten(evals), coset_index, proof["commit_phase_merkle_caps"][i], rp["steps"][i]["merkle_proof"]), \
                "FRI layer Merkle proof"
            subgroup_x = pow(subgroup_x, arity, P)
            xi = coset_index
        acc = (0, 0)
        for c in reversed(proof["final_poly"]):
            acc = ext_add(ext_mul(acc, (subgroup_x, 0)), c)
        assert tuple(acc) == tuple(old_eval), "Final polynomial evaluation is invalid."
    return True


def verify(hasher, circuit, proof):
    """plonk/verifier.rs:15-120. Returns True or raises AssertionError."""
    ext_mul, ext_sub, ext_pow = fri_ref.ext_mul, fri_ref.ext_sub, fri_ref.ext_pow
    pih = pyref.hash_no_pad(proof["public_inputs"])
    chal = get_challenges(hasher, circuit, proof, pih)
    op = proof["openings"]
    zeta = chal["plonk_zeta"]
    vanishing = prove_ref.eval_vanishing_poly(circuit, zeta, op, pih, chal["plonk_betas"], chal["plonk_gammas"], chal["plonk_alphas"])
    zeta_pow_deg = ext_pow(zeta, 1 << circuit["degree_bits"])
    z_h_zeta = ext_sub(zeta_pow_deg, (1, 0))
    qdf = circuit["quotient_degree_factor"]
    assert len(op["quotient_polys"]) == circuit["num_challenges"] * qdf
    for i in range(circuit["num_challenges"]):
        t = fri_ref.reduce_with_powers_ext(op["quotient_polys"][i * qdf : (i + 1) * qdf], zeta_pow_deg)
        assert vanishing[i] == ext_mul(z_h_zeta, t), "vanishing(zeta) != Z_H(zeta) * t(zeta)"
    caps = [circuit["constants_sigmas"]["cap"], proof["wires_cap"], proof["plonk_zs_partial_products_cap"], proof["quotient_polys_cap"]]
    return verify_fri_proof(hasher, prove_ref.fri_instance(circuit, zeta), prove_ref.fri_openings(op), chal["fri_challenges"], caps,
                            proof["opening_proof"], circuit["degree_bits"], circuit["fri_params"])


# ---------------------------------------------------------------- wire format
def _u64(xs):
    return np.array([int(x) % P for x in xs], dtype="<u8").tobytes()


def _flat_ext(v):
    return [c for e in v for c in e]


def proof_bytes(hasher, proof):
    """write_proof_with_public_inputs (util/serialization.rs:641-689); write_hash = GenericHashOut::to_bytes (:537-543)"""
    hashes = lambda hs: b"".join(hasher.to_bytes(h) for h in hs)  # noqa: E731
    out = [hashes(cap) for cap in (proof["wires_cap"], proof["plonk_zs_partial_products_cap"], proof["quotient_polys_cap"])]
    op = proof["openings"]
    for k in ("constants", "plonk_sigmas", "wires", "plonk_zs", "plonk_zs_next", "partial_products", "quotient_polys"):
        out.append(_u64(_flat_ext(op[k])))
    fp = proof["opening_proof"]
    out += [hashes(cap) for cap in fp["commit_phase_merkle_caps"]]
    for rnd in fp["query_round_proofs"]:
        for evals, sib in rnd["initial_trees_proof"]:
            out += [_u64(evals), bytes([len(sib)]), hashes(sib)]
        for st in rnd["steps"]:
            out += [_u64(_flat_ext(st["evals"])), bytes([len(st["merkle_proof"])]), hashes(st["merkle_proof"])]
    out += [_u64(_flat_ext(fp["final_poly"])), _u64([fp["pow_witness"]]), _u64(proof["public_inputs"])]
    return b"".join(out)


def count_hashes(proof):
    """how many hashes a proof carries: caps and Merkle siblings"""
    fp = proof["opening_proof"]
    k = sum(len(proof[c]) for c in ("wires_cap", "plonk_zs_partial_products_cap", "quotient_polys_cap"))
    k += sum(len(cap) for cap in fp["commit_phase_merkle_caps"])
    for rnd in fp["query_round_proofs"]:
        k += sum(len(sib) for _, sib in rnd["initial_trees_proof"]) + sum(len(st["merkle_proof"]) for st in rnd["steps"])
    return k
