"""The multi-table STARK prover and verifier of the reference's evm crate restated in pure Python (TEST INFRASTRUCTURE ONLY), without
anything EVM-specific: the independent reference gl_stark_tables_prove, gl_stark_tables_ctl_zs and gl_stark_tables_quotient_polys
are held against.

    prove_tables         evm/src/prover.rs:66-421 (prove_with_traces, prove_single_table, compute_quotient_polys)
    CTL data             evm/src/cross_table_lookup.rs:29-451 (Column::eval, cross_table_lookup_data, partial_products,
                         eval_cross_table_lookup_checks)
    the FRI instance     evm/src/stark.rs:83-142; the openings evm/src/proof.rs:190-257
    compact              plonky2/src/iop/challenger.rs:149-155

The algebra, the commits, prove_openings, verify_fri_proof, the Consumer and the program interpreter are tests/stark_ref.py's and
tests/generic_prove_ref.py's. A system here is an object with `tables` (STARKs as stark_ref takes them: num_columns,
constraint_degree, pairs, instrs / immediates, closure; num_public_inputs 0), `lookups` (objects with looking_tables,
looked_table, default; a table-with-columns has table, columns, filter_column; a column has terms [(column, coeff)] and
constant) and `ctl_closures`, per table the CTL checks of that table written out by hand:
ctl_closures[k](F, local, nxt, local_zs, next_zs, challenges, consumer). Every function that evaluates constraints takes
`evaluator`: "program" runs the register program and the generic CTL evaluator over the description, "closure" the hand-written
closures; the two must agree (tests/test_ctl_ref.py).

verify_tables checks (1) every table's quotient identity at zeta with the CTL checks over Ext, (2) every table's FRI proof over the
three batches, (3) the cross-table product: per lookup and per challenge c
    prod looking z_last == looked z_last * combine_c(default)^(sum looking n - looked n),
with challenge c itself and no default factor for a lookup with filters or without a default. The reference's
verify_cross_table_lookups (cross_table_lookup.rs:613-622) indexes the challenge by the LOOKUP's number and skips lookups without a
default; this file checks what the argument means, not that.

The wire format is the one include/plonky2_hip.h defines for gl_stark_tables_prove, written here from the header's text."""
import generic_prove_ref as gr
import stark_ref as sr
from oracle import fri_ref, plonk_ref, pyref

P = pyref.P
Base, Ext, Consumer = sr.Base, sr.Ext, sr.Consumer


def compact(ch):
    """Challenger::compact (challenger.rs:149-155) on a fri_ref.Challenger"""
    if ch.input_buffer:
        ch.duplexing()
    ch.output_buffer = []
    return list(ch.sponge_state)


# ---------------------------------------------------------------- columns, Zs
def eval_column(F, col, row):
    """Column::eval (cross_table_lookup.rs:100-119)"""
    acc = F.lift(col.constant)
    for c, k in col.terms:
        acc = F.add(acc, F.mul(row[c], F.lift(k)))
    return acc


def combine(F, values, challenge):
    """GrandProductChallenge::combine (evm/src/permutation.rs:61-73): reduce_with_powers(values, beta) + gamma"""
    beta, gamma = challenge
    acc = F.zero
    for v in reversed(values):
        acc = F.add(F.mul(acc, F.lift(beta)), v)
    return F.add(acc, F.lift(gamma))


def ctl_zs_order(lookups, num_challenges, table):
    """the CTL Zs of `table` as cross_table_lookup_data appends them (:245-309): (lookup index, challenge index, TWC)"""
    out = []
    for li, lk in enumerate(lookups):
        for c in range(num_challenges):
            for twc in lk.looking_tables:
                if twc.table == table:
                    out.append((li, c, twc))
            if lk.looked_table.table == table:
                out.append((li, c, lk.looked_table))
    return out


def partial_products(trace, twc, challenge):
    """cross_table_lookup.rs:314-341 -> [n] values; `trace` [num_columns][n] of any u64"""
    n = len(trace[0])
    z, acc = [], 1
    for r in range(n):
        row = [int(col[r]) % P for col in trace]
        f = 1 if twc.filter_column is None else eval_column(Base, twc.filter_column, row)
        if f == 1:
            acc = acc * combine(Base, [eval_column(Base, c, row) for c in twc.columns], challenge) % P
        else:
            assert f == 0, "Non-binary filter?"
        z.append(acc)
    return z


def ctl_z_polys(lookups, num_challenges, table, trace, challenges):
    """the CTL Zs of one table, [num_ctl_zs][n]"""
    return [partial_products(trace, twc, challenges[c]) for _, c, twc in ctl_zs_order(lookups, num_challenges, table)]


def product_identity_holds(lookups, traces, challenge):
    """the debug_assert of cross_table_lookup_data (:268-289) for one challenge, over all lookups"""
    for lk in lookups:
        looking = 1
        for twc in lk.looking_tables:
            looking = looking * partial_products(traces[twc.table], twc, challenge)[-1] % P
        looked = partial_products(traces[lk.looked_table.table], lk.looked_table, challenge)[-1]
        if lk.default is not None:
            extra = sum(len(traces[t.table][0]) for t in lk.looking_tables) - len(traces[lk.looked_table.table][0])
            looked = looked * pow(combine(Base, [int(x) % P for x in lk.default], challenge), extra, P) % P
        if looking != looked:
            return False
    return True


def eval_ctl_checks(F, local, nxt, ctl_vars, consumer):
    """eval_cross_table_lookup_checks (:410-451); ctl_vars: (local_z, next_z, challenge, twc) per CTL Z"""
    for local_z, next_z, challenge, twc in ctl_vars:
        def select(row):
            x = combine(F, [eval_column(F, c, row) for c in twc.columns], challenge)
            if twc.filter_column is None:
                return x
            f = eval_column(F, twc.filter_column, row)
            return F.sub(F.add(F.mul(f, x), F.one), f)

        consumer.constraint_first_row(F.sub(local_z, select(local)))
        consumer.constraint_transition(F.sub(next_z, F.mul(local_z, select(nxt))))


def eval_vanishing_poly(F, system, table, num_challenges, local, nxt, local_zs, next_zs, perm_sets, ctl_challenges, consumer, evaluator):
    """evm/src/vanishing_poly.rs:16-44: the STARK's constraints, the permutation checks, the CTL checks; local_zs / next_zs: the whole
    Zs oracle's row (permutation Zs, then CTL Zs)"""
    stark = system.tables[table]
    nperm = sr.num_zs(stark, num_challenges)
    sr.eval_constraints(F, stark, local, nxt, [], consumer, evaluator)
    if stark.pairs:
        sr.eval_permutation_checks(F, stark, num_challenges, local, local_zs[:nperm], next_zs[:nperm], perm_sets, consumer)
    if evaluator == "program":
        order = ctl_zs_order(system.lookups, num_challenges, table)
        ctl_vars = [(local_zs[nperm + i], next_zs[nperm + i], ctl_challenges[c], twc) for i, (_, c, twc) in enumerate(order)]
        eval_ctl_checks(F, local, nxt, ctl_vars, consumer)
    else:
        system.ctl_closures[table](F, local, nxt, local_zs[nperm:], next_zs[nperm:], ctl_challenges, consumer)


# ---------------------------------------------------------------- prove
def compute_quotient_polys(system, table, num_challenges, degree_bits, rate_bits, trace_leaves, zs_leaves, perm_sets, ctl_challenges, alphas,
                           evaluator="program"):
    """evm/src/prover.rs:425-558 -> [num_challenges][n << qdb] coefficients; the leaves are rows reverse_bits(idx) of the LDEs (any
    words do: nothing here needs low degree); zs_leaves None for a table without any Z"""
    stark = system.tables[table]
    n = 1 << degree_bits
    qdb = (sr.quotient_degree_factor(stark) - 1).bit_length()
    assert qdb <= rate_bits, "Having constraints of degree higher than the rate is not supported yet."
    step, next_step, size, bits = 1 << (rate_bits - qdb), 1 << qdb, n << qdb, degree_bits + rate_bits
    selector = lambda k: pyref.fast_ntt([1 if i == k else 0 for i in range(n)], inverse=True)  # noqa: E731
    lagrange_first, lagrange_last = sr._coset_fft(selector(0), size), sr._coset_fft(selector(n - 1), size)
    last = pow(pyref.root_of_unity(degree_bits), P - 2, P)
    w = pyref.root_of_unity(degree_bits + qdb)
    values = [[] for _ in range(num_challenges)]
    x = pyref.GENERATOR
    for i in range(size):
        row, row_next = pyref.reverse_bits(i * step, bits), pyref.reverse_bits(((i + next_step) % size) * step, bits)
        consumer = Consumer(Base, alphas, (x - last) % P, lagrange_first[i], lagrange_last[i])
        zs, zs_next = ([], []) if zs_leaves is None else (zs_leaves[row], zs_leaves[row_next])
        eval_vanishing_poly(Base, system, table, num_challenges, trace_leaves[row], trace_leaves[row_next], zs, zs_next, perm_sets, ctl_challenges,
                            consumer, evaluator)
        z_h_inv = pow((pow(x, n, P) - 1) % P, P - 2, P)
        for k, acc in enumerate(consumer.accs):
            values[k].append(acc * z_h_inv % P)
        x = x * w % P
    return [sr._coset_ifft(v) for v in values]


def fri_instance(stark, num_challenges, num_ctl_zs, zeta, degree_bits):
    """evm/src/stark.rs:83-142: everything at zeta; trace and all Zs at g zeta; the CTL Zs at 1 / g"""
    nperm = sr.num_zs(stark, num_challenges)
    sizes = [stark.num_columns, nperm + num_ctl_zs, sr.quotient_degree_factor(stark) * num_challenges]
    infos = [[(oi, pi) for pi in range(k)] for oi, k in enumerate(sizes)]
    g = pyref.root_of_unity(degree_bits)
    return dict(batches=[(zeta, infos[0] + infos[1] + infos[2]), (fri_ref.ext_mul((g, 0), zeta), infos[0] + infos[1]),
                         ((pow(g, P - 2, P), 0), infos[1][nperm:])])


def to_fri_openings(op):
    """evm/src/proof.rs:226-257"""
    return [op["local_values"] + op["permutation_ctl_zs"] + op["quotient_polys"], op["next_values"] + op["permutation_ctl_zs_next"],
            [(x, 0) for x in op["ctl_zs_last"]]]


def prove_single_table(hasher, system, table, num_challenges, fri_params, trace, trace_c, ctl_zs, ctl_challenges, ch, evaluator):
    """evm/src/prover.rs:245-421"""
    stark = system.tables[table]
    rate_bits, cap_height = fri_params["rate_bits"], fri_params["cap_height"]
    n = len(trace[0])
    degree_bits = pyref.log2_strict(n)
    assert sum(fri_params["reduction_arity_bits"]) <= degree_bits + rate_bits - cap_height, "FRI total reduction arity is too large."
    qdf = sr.quotient_degree_factor(stark)
    compact(ch)
    perm_sets, z_polys = None, []
    if stark.pairs:
        perm_sets = sr.get_n_permutation_challenge_sets(ch, num_challenges, qdf)
        z_polys = sr.compute_permutation_z_polys(stark, num_challenges, trace, perm_sets)
    nperm = len(z_polys)
    z_polys = z_polys + ctl_zs
    assert z_polys, "No CTL?"
    zs_c = gr.commit_from_values(hasher, z_polys, rate_bits, cap_height)
    gr.observe_cap(hasher, ch, zs_c["cap"])
    alphas = ch.get_n_challenges(num_challenges)
    quotient_polys = compute_quotient_polys(system, table, num_challenges, degree_bits, rate_bits, trace_c["leaves"], zs_c["leaves"], perm_sets,
                                            ctl_challenges, alphas, evaluator)
    chunks = []
    for q in quotient_polys:
        assert all(c == 0 for c in q[n * qdf :]), "Quotient has failed, the vanishing polynomial is not divisible by Z_H"
        chunks += [q[k : k + n] for k in range(0, n * qdf, n)]
    quot_c = gr.commit_from_coeffs(hasher, chunks, rate_bits, cap_height)
    gr.observe_cap(hasher, ch, quot_c["cap"])
    zeta = ch.get_extension_challenge()
    assert fri_ref.ext_pow(zeta, n) != (1, 0), "Opening point is in the subgroup."
    g = pyref.root_of_unity(degree_bits)
    g_zeta = fri_ref.ext_mul((g, 0), zeta)
    ev = lambda c, z: [plonk_ref.eval_ext2(p, z) for p in c["polynomials"]]  # noqa: E731
    g_inv = pow(g, P - 2, P)
    base_eval = lambda p: sum(c * pow(g_inv, i, P) for i, c in enumerate(p)) % P  # noqa: E731
    openings = dict(local_values=ev(trace_c, zeta), next_values=ev(trace_c, g_zeta), permutation_ctl_zs=ev(zs_c, zeta),
                    permutation_ctl_zs_next=ev(zs_c, g_zeta), ctl_zs_last=[base_eval(p) for p in zs_c["polynomials"][nperm:]],
                    quotient_polys=ev(quot_c, zeta))
    for batch in to_fri_openings(openings):
        ch.observe_extension_elements(batch)
    instance = fri_instance(stark, num_challenges, len(ctl_zs), zeta, degree_bits)
    opening_proof = gr.prove_openings(hasher, instance, [trace_c, zs_c, quot_c], ch, fri_params)
    return dict(trace_cap=trace_c["cap"], permutation_ctl_zs_cap=zs_c["cap"], quotient_polys_cap=quot_c["cap"], openings=openings,
                opening_proof=opening_proof)


def get_ctl_challenges(ch, num_challenges):
    """get_grand_product_challenge_set (evm/src/permutation.rs:190-206): (beta, gamma) per challenge"""
    return [tuple(ch.get_n_challenges(2)) for _ in range(num_challenges)]


def prove_tables(hasher, system, num_challenges, fri_params, traces, evaluator="program", check=True):
    """prove_with_traces (evm/src/prover.rs:66-149). `fri_params`: one dict per table (they differ in reduction_arity_bits only);
    `traces`: per table [num_columns][n] values. check=False skips the product debug_assert (for traces that break a lookup)."""
    traces = [[[int(x) % P for x in col] for col in t] for t in traces]
    commits = [gr.commit_from_values(hasher, t, fp["rate_bits"], fp["cap_height"]) for t, fp in zip(traces, fri_params)]
    ch = fri_ref.Challenger()
    for c in commits:
        gr.observe_cap(hasher, ch, c["cap"])
    ctl_challenges = get_ctl_challenges(ch, num_challenges)
    if check:
        assert all(product_identity_holds(system.lookups, traces, c) for c in ctl_challenges), "the CTL product identity"
    ctl_zs = [ctl_z_polys(system.lookups, num_challenges, k, traces[k], ctl_challenges) for k in range(len(traces))]
    return [prove_single_table(hasher, system, k, num_challenges, fri_params[k], traces[k], commits[k], ctl_zs[k], ctl_challenges, ch, evaluator)
            for k in range(len(traces))]


# ---------------------------------------------------------------- verify
def verify_tables(hasher, system, num_challenges, fri_params, proofs, evaluator="program"):
    """verify_proof (evm/src/verifier.rs) without public values, with the product check described at the top. True or AssertionError."""
    assert len(proofs) == len(system.tables)
    ch = fri_ref.Challenger()
    for p in proofs:
        gr.observe_cap(hasher, ch, p["trace_cap"])
    ctl_challenges = get_ctl_challenges(ch, num_challenges)
    for k, (stark, proof, fp) in enumerate(zip(system.tables, proofs, fri_params)):
        op = proof["openings"]
        order = ctl_zs_order(system.lookups, num_challenges, k)
        nperm, qdf = sr.num_zs(stark, num_challenges), sr.quotient_degree_factor(stark)
        lde_bits = fp["cap_height"] + len(proof["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"][0][1])
        degree_bits = lde_bits - fp["rate_bits"]
        assert len(op["local_values"]) == len(op["next_values"]) == stark.num_columns and len(op["quotient_polys"]) == qdf * num_challenges
        assert len(op["permutation_ctl_zs"]) == len(op["permutation_ctl_zs_next"]) == nperm + len(order) and len(op["ctl_zs_last"]) == len(order)
        assert len(proof["trace_cap"]) == len(proof["permutation_ctl_zs_cap"]) == len(proof["quotient_polys_cap"]) == 1 << fp["cap_height"]
        # get_challenges (evm/src/get_challenges.rs), the one transcript running on
        compact(ch)
        perm_sets = sr.get_n_permutation_challenge_sets(ch, num_challenges, qdf) if stark.pairs else None
        gr.observe_cap(hasher, ch, proof["permutation_ctl_zs_cap"])
        alphas = ch.get_n_challenges(num_challenges)
        gr.observe_cap(hasher, ch, proof["quotient_polys_cap"])
        zeta = ch.get_extension_challenge()
        for batch in to_fri_openings(op):
            ch.observe_extension_elements(batch)
        fri_chal = gr.fri_challenges(hasher, ch, proof["opening_proof"], degree_bits, fp)
        # the quotient identity at zeta
        l_0, l_last = sr.eval_l_0_and_l_last(degree_bits, zeta)
        last = pow(pyref.root_of_unity(degree_bits), P - 2, P)
        consumer = Consumer(Ext, alphas, fri_ref.ext_sub(zeta, (last, 0)), l_0, l_last)
        eval_vanishing_poly(Ext, system, k, num_challenges, op["local_values"], op["next_values"], op["permutation_ctl_zs"],
                            op["permutation_ctl_zs_next"], perm_sets, ctl_challenges, consumer, evaluator)
        zeta_pow_deg = fri_ref.ext_pow(zeta, 1 << degree_bits)
        z_h_zeta = fri_ref.ext_sub(zeta_pow_deg, (1, 0))
        for i in range(num_challenges):
            t = fri_ref.reduce_with_powers_ext(op["quotient_polys"][i * qdf : (i + 1) * qdf], zeta_pow_deg)
            assert tuple(consumer.accs[i]) == tuple(fri_ref.ext_mul(z_h_zeta, t)), "Mismatch between evaluation and opening of quotient polynomial"
        caps = [proof["trace_cap"], proof["permutation_ctl_zs_cap"], proof["quotient_polys_cap"]]
        gr.verify_fri_proof(hasher, fri_instance(stark, num_challenges, len(order), zeta, degree_bits), to_fri_openings(op), fri_chal, caps,
                            proof["opening_proof"], degree_bits, fp)
    # the cross-table product, per lookup and per challenge
    degree = [1 << (fp["cap_height"] + len(p["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"][0][1]) - fp["rate_bits"])
              for p, fp in zip(proofs, fri_params)]
    cursor = [iter(p["openings"]["ctl_zs_last"]) for p in proofs]
    for lk in system.lookups:
        for c in range(num_challenges):
            looking = 1
            for twc in lk.looking_tables:
                looking = looking * next(cursor[twc.table]) % P
            looked = next(cursor[lk.looked_table.table])
            if lk.default is not None:
                extra = sum(degree[t.table] for t in lk.looking_tables) - degree[lk.looked_table.table]
                looked = looked * pow(combine(Base, [int(x) % P for x in lk.default], ctl_challenges[c]), extra, P) % P
            assert looking == looked, "cross-table lookup: the products of the looking and of the looked table differ"
    return True


# ---------------------------------------------------------------- wire format (include/plonky2_hip.h, gl_stark_tables_prove)
def proofs_bytes(hasher, proofs):
    hashes = lambda hs: b"".join(hasher.to_bytes(h) for h in hs)  # noqa: E731
    u64, flat = sr._u64, sr._flat_ext
    out = []
    for proof in proofs:
        out += [hashes(proof["trace_cap"]), hashes(proof["permutation_ctl_zs_cap"]), hashes(proof["quotient_polys_cap"])]
        op = proof["openings"]
        for k in ("local_values", "next_values", "permutation_ctl_zs", "permutation_ctl_zs_next"):
            out.append(u64(flat(op[k])))
        out += [u64(op["ctl_zs_last"]), u64(flat(op["quotient_polys"]))]
        fp = proof["opening_proof"]  # write_fri_proof (util/serialization.rs)
        out += [hashes(cap) for cap in fp["commit_phase_merkle_caps"]]
        for rnd in fp["query_round_proofs"]:
            for evals, sib in rnd["initial_trees_proof"]:
                out += [u64(evals), bytes([len(sib)]), hashes(sib)]
            for st in rnd["steps"]:
                out += [u64(flat(st["evals"])), bytes([len(st["merkle_proof"])]), hashes(st["merkle_proof"])]
        out += [u64(flat(fp["final_poly"])), u64([fp["pow_witness"]])]
    return b"".join(out)
