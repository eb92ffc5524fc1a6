// See prover.h.  Stage order and span names follow prove_with_preprocessed
// (eon-uni-stark/src/prover.rs): commit (186-187) -> quotient domain (307-308) -> LDE (315) ->
// quotient_values (328-342) -> commit_quotient (371-372) -> open at [zeta, zeta h] and [zeta] per
// chunk (416-442).  With preprocessed columns (setup_preprocessed, preprocessed.rs:47-94) their
// commitment is observed after the trace's (203-205), their evaluations on the quotient domain are
// read by the constraints (321-322) and they are opened last, at [zeta, zeta h] (431).  With lookups
// the permutation challenges are sampled after the public values (214-216), the permutation trace is
// generated, committed and observed (238-273) before alpha, and opened right after the trace (427-437).
//
// Lane sharding: the vectorized AIR evaluates its lanes one after another
// (poseidon2-air/src/vectorized.rs:259-274), so lane v owns columns [164 v, 164 v + 164) and
// constraints [K v, K v + K), K = 160.  A rank proving lanes [l0, l1) commits, extends and opens
// its own columns, and its folder accumulator times alpha^(K (VL - l1)) is its exact share of the
// full one (folder.rs:81-85).  The partials are all-gathered (Q x 32 B, the one data-path
// exchange) and combined on device; the per-column results are all-gathered at the end.
//
// Column sharding: a generic AIR's constraints read every column of a row, so a rank
// that owns a column range (eon_shard_column_range) commits, extends and opens its columns, but
// cannot evaluate the quotient on them alone.  The ranks exchange their extended columns once as
// row blocks (eon_shard_pack_rows_dev, all_to_all, eon_shard_unpack_cols_dev): rank r then holds
// every column of ITS rows of the quotient domain (eon_shard_row_range) plus the 2^log_qd rows its
// "next" rows reach into, evaluates the quotient there (eon_quotient_values_rows_dev), and the row
// blocks are all-gathered.  From there the tail is the lane-sharded one.
#include "prover.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <thread>

namespace eon_host {

uint32_t log_quotient_degree(uint32_t max_constraint_degree) {
    const uint32_t d = (max_constraint_degree > 2 ? max_constraint_degree : 2) - 1;
    uint32_t b = 0;
    while ((1u << b) < d) b++;
    return b;
}

namespace {

// per-column record of the final all-gather: commitment (8) | value at zeta (4) | value at zeta h
// (4) | witness at zeta (8) | witness at zeta h (8), in u64
constexpr uint32_t RECORD = 32;

void all_gather(eon_ctx* ctx, const eon_collective* coll, const void* send, void* recv, uint64_t bytes) {
    const int rc = coll->all_gather(coll->user, send, recv, bytes, eon_ctx_stream(ctx));
    if (rc != 0) throw Error(EON_E_DEVICE, "collective all_gather failed (" + std::to_string(rc) + ")");
}

void all_to_all(eon_ctx* ctx, const eon_collective* coll, const void* send, void* recv, uint64_t bytes) {
    const int rc = coll->all_to_all(coll->user, send, recv, bytes, eon_ctx_stream(ctx));
    if (rc != 0) throw Error(EON_E_DEVICE, "collective all_to_all failed (" + std::to_string(rc) + ")");
}

void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Error(EON_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

uint32_t AirRef::width() const {
    if (p2) return eon_p2air_width(p2);
    eon_air_program_stats st{};
    if (prog && eon_air_program_info(prog, &st) == EON_OK) return st.width;
    return 0;
}

std::unique_ptr<Preprocessed> setup_preprocessed(KzgPcs& pcs, const eon_fr* pre_trace, uint64_t height,
                                                 uint32_t width) {
    pcs.require_prover("setup_preprocessed");
    eon_ctx* ctx = pcs.ctx();
    if (width == 0)  // preprocessed.rs:68-70 returns None: the caller proves without one
        throw Error(EON_E_SHAPE, "the preprocessed trace has no columns: prove without preprocessed data");
    if (!pre_trace) throw Error(EON_E_ARG, "null preprocessed trace");
    if (height == 0 || (height & (height - 1)))
        throw Error(EON_E_SHAPE, "preprocessed trace height must be a power of two");
    auto pp = std::make_unique<Preprocessed>();
    pp->pcs = &pcs;
    pp->width = width;
    pp->degree_bits = 63 - __builtin_clzll(height);
    // the handle owns its evaluations (the reference's ProverData keeps them, kzg/src/pcs.rs:46-63)
    DeviceMatrix evals = DeviceMatrix::alloc(height, width);
    hipStream_t st = static_cast<hipStream_t>(eon_ctx_stream(ctx));
    hip_ok(hipMemcpyAsync(evals.mutable_data(), pre_trace, height * width * sizeof(eon_fr), hipMemcpyDeviceToDevice,
                          st),
           "preprocessed trace");
    std::vector<std::pair<Domain, DeviceMatrix>> ev;
    ev.emplace_back(pcs.natural_domain_for_degree(height), std::move(evals));
    std::vector<std::vector<eon_g1_affine>> commit;
    pcs.commit(std::move(ev), commit, pp->data);  // preprocessed.rs:79-80
    pp->commitment = std::move(commit[0]);
    return pp;
}

Proof prove(KzgPcs& pcs, const AirRef& air, const eon_fr* trace, uint64_t height, const Fr& alpha_in,
            const Fr& zeta_in, uint32_t max_constraint_degree, const eon_collective* shard,
            DuplexChallenger* challenger, const Preprocessed* pp, const LookupInputs* lookups,
            ConstraintCheck* constraint_check, BatchedOpening* batched) {
    pcs.require_prover("prove");
    if (batched && shard && shard->world > 1)
        throw Error(EON_E_ARG, "the batched opening is not lane-sharded: prove on one device or per column");
    if (batched && !challenger && !batched->have_gamma)
        throw Error(EON_E_ARG, "the batched opening without a challenger needs gamma "
                               "(eon_kzg_pcs_set_opening_challenges)");
    eon_ctx* ctx = pcs.ctx();
    using clock = std::chrono::steady_clock;
    auto tick = [&] {
        check(ctx, eon_ctx_synchronize(ctx), "eon_ctx_synchronize");
        return clock::now();
    };
    auto ms = [](clock::time_point a, clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    if (height == 0 || (height & (height - 1))) throw Error(EON_E_SHAPE, "trace height must be a power of two");
    if ((air.p2 == nullptr) == (air.prog == nullptr)) throw Error(EON_E_ARG, "exactly one of p2air / program");
    if (air.n_public && !air.publics) throw Error(EON_E_ARG, "null public values");
    if (air.p2 && air.n_public) throw Error(EON_E_SHAPE, "the Poseidon2-AIR has no public values");
    if (air.p2) constraint_check = nullptr;  // the fused path has no program to check
    uint32_t width = air.width();  // of `trace`: the AIR's, or (column-sharded) the rank's range
    const uint32_t local_vl = air.p2 ? eon_p2air_vector_len(air.p2) : 1;
    const uint32_t k_lane = air.p2 ? eon_p2air_constraints_per_perm(air.p2) : 0;
    if (shard && shard->world <= 1) shard = nullptr;
    if (shard && (!shard->all_gather || shard->rank >= shard->world))
        throw Error(EON_E_ARG, "invalid collective");
    const uint32_t world = shard ? shard->world : 1, rank = shard ? shard->rank : 0;
    // A program is sharded by columns.  What it cannot do is refused here, from arguments that are
    // the same on every rank and before the first collective call, so no rank is left waiting.
    const bool col_shard = shard && air.prog;
    const uint32_t full_width = col_shard ? width : width * world;
    if (col_shard) {
        if (!shard->all_to_all) throw Error(EON_E_ARG, "the column-sharded prove needs a collective with all_to_all");
        if (world > full_width)
            throw Error(EON_E_ARG, "column sharding: more ranks than columns (" + std::to_string(world) + " ranks, " +
                                       std::to_string(full_width) + " columns)");
        if (pp || eon_air_program_preprocessed_width(air.prog) > 0)
            throw Error(EON_E_ARG, "preprocessed columns are not column-sharded: prove on one device");
        if (lookups || eon_air_program_permutation_width(air.prog) > 0)
            throw Error(EON_E_ARG, "lookups are not column-sharded: prove on one device");
        if (constraint_check)
            throw Error(EON_E_ARG, "check_constraints is not column-sharded: it reads whole rows of the trace; "
                                   "switch it off or prove on one device");
        uint32_t col0 = 0;  // `trace` is the slice itself: its first column's position is the records' business
        if (eon_shard_column_range(full_width, world, rank, &col0, &width) != EON_OK)
            throw Error(EON_E_ARG, "eon_shard_column_range");
    }
    // columns of rank g in the full proof, and the (padded) per-rank slot count of the exchanges
    auto cols_of = [&](uint32_t g, uint32_t* c0, uint32_t* wl) {
        if (!col_shard) {
            *c0 = g * width;
            *wl = width;
        } else if (eon_shard_column_range(full_width, world, g, c0, wl) != EON_OK) {
            throw Error(EON_E_ARG, "eon_shard_column_range");
        }
    };
    const uint32_t slots = col_shard ? (full_width + world - 1) / world : width;
    const uint32_t vector_len = local_vl * world;
    const uint32_t log_n = 63 - __builtin_clzll(height);
    // the preprocessed data against the AIR's declaration (prover.rs:58-88: the reference panics)
    const uint32_t pre_width = air.prog ? eon_air_program_preprocessed_width(air.prog) : 0;
    if (pre_width > 0 && !pp)
        throw Error(EON_E_ARG, "the program has preprocessed columns but no preprocessed data was provided "
                               "(eon_setup_preprocessed, eon_prove_air_pp)");
    if (pp) {
        if (shard) throw Error(EON_E_ARG, "preprocessed columns are not lane-sharded");
        if (pp->pcs != &pcs) throw Error(EON_E_ARG, "the preprocessed data was committed with another pcs");
        if (pp->degree_bits != log_n)
            throw Error(EON_E_SHAPE, "preprocessed degree_bits " + std::to_string(pp->degree_bits) +
                                         " differs from the trace's " + std::to_string(log_n));
        if (pp->width != pre_width)
            throw Error(EON_E_SHAPE, "preprocessed width " + std::to_string(pp->width) +
                                         " differs from the AIR's " + std::to_string(pre_width));
    }
    // lookups (prover.rs:90-95): one running-sum column and two challenges each
    const uint32_t perm_width = air.prog ? eon_air_program_permutation_width(air.prog) : 0;
    const uint32_t n_challenges = air.prog ? eon_air_program_num_challenges(air.prog) : 0;
    if (perm_width > 0 && !lookups)
        throw Error(EON_E_ARG, "the program has lookups (permutation columns): prove it with eon_prove_air_lk");
    if (perm_width > 0 && eon_air_program_num_lookups(air.prog) != perm_width)
        throw Error(EON_E_ARG, "the program has permutation columns but no lookup description");
    if (perm_width > 0 && !challenger && !lookups->challenges)
        throw Error(EON_E_ARG, "null permutation challenges");
    // get_log_quotient_degree (prover.rs:150-157): the program's own constraint degrees
    const uint32_t log_qd =
        air.prog ? eon_air_program_log_quotient_degree(air.prog, 0) : log_quotient_degree(max_constraint_degree);
    const uint32_t num_chunks = 1u << log_qd;
    hipStream_t st = static_cast<hipStream_t>(eon_ctx_stream(ctx));

    Proof proof;
    proof.degree_bits = log_n;
    const Domain trace_domain = pcs.natural_domain_for_degree(height);

    auto t0 = tick();
    std::vector<std::vector<eon_g1_affine>> trace_commit;
    std::vector<MatrixProverData> trace_data;
    const Domain quotient_domain = trace_domain.create_disjoint_domain(1ull << (log_n + log_qd));
    const uint64_t q_rows = quotient_domain.size();
    DeviceMatrix lde, pre_lde, perm_lde;
    std::vector<std::vector<eon_g1_affine>> perm_commit;
    std::vector<MatrixProverData> perm_data;
    std::vector<Fr> perm_challenges(n_challenges);
    if (perm_width > 0 && !challenger)
        for (uint32_t i = 0; i < n_challenges; i++) perm_challenges[i] = Fr::from_abi(lookups->challenges[i]);
    clock::time_point t1, t2;
    {
        std::vector<std::pair<Domain, DeviceMatrix>> ev;
        ev.emplace_back(trace_domain, DeviceMatrix::borrow(trace, height, width));
        pcs.commit_coeffs(std::move(ev), trace_data);
    }
    pcs.commit_columns(trace_data, 0, trace_commit);
    t1 = tick();
    // Fiat-Shamir up to alpha (prover.rs:196-208, 300) on a host thread while the device extends
    // the trace: sharded, every rank observes the full commitment (all-gathered in rank = lane
    // order first)
    Fr alpha = alpha_in;
    std::thread fs_thread;
    std::vector<eon_g1_affine> full_commit;
    if (challenger) {
        if (shard) {
            // padded slots (column ranges differ by one), trimmed to the full width in rank order
            const uint64_t bytes = (uint64_t)slots * sizeof(eon_g1_affine);
            DeviceBuffer send(bytes), recv(bytes * world);
            if (slots != width) hip_ok(hipMemsetAsync(send.get(), 0, bytes, st), "commit");
            hip_ok(hipMemcpyAsync(send.get(), trace_commit[0].data(), (uint64_t)width * sizeof(eon_g1_affine),
                                  hipMemcpyHostToDevice, st),
                   "commit");
            all_gather(ctx, shard, send.get(), recv.get(), bytes);
            std::vector<eon_g1_affine> all((uint64_t)slots * world);
            hip_ok(hipMemcpyAsync(all.data(), recv.get(), bytes * world, hipMemcpyDeviceToHost, st), "commit");
            hip_ok(hipStreamSynchronize(st), "commit");
            full_commit.resize(full_width);
            for (uint32_t g = 0; g < world; g++) {
                uint32_t c0, wl;
                cols_of(g, &c0, &wl);
                std::copy_n(all.begin() + (uint64_t)g * slots, wl, full_commit.begin() + c0);
            }
        } else {
            full_commit = trace_commit[0];
        }
        fs_thread = std::thread([&] {
            challenger->observe(fr_from_u64(log_n));  // log_ext_degree (ZK off)
            challenger->observe(fr_from_u64(log_n));  // log_degree
            challenger->observe(fr_from_u64(pre_width));  // preprocessed width
            challenger->observe_g1(full_commit.data(), full_commit.size());
            if (pp) challenger->observe_g1(pp->commitment.data(), pp->commitment.size());  // prover.rs:203-205
            for (uint32_t i = 0; i < air.n_public; i++)  // observe_slice(public_values), prover.rs:208
                challenger->observe(Fr::from_abi(air.publics[i]));
            if (perm_width > 0)  // prover.rs:214-216; alpha follows the permutation commitment
                for (uint32_t i = 0; i < n_challenges; i++) perm_challenges[i] = challenger->sample();
            else if (!constraint_check)
                alpha = challenger->sample();  // with the check on, after it (below)
        });
    }
    // the trace LDE (prover.rs:315) while the host thread runs the transcript up to alpha
    DeviceMatrix window;   // column-sharded: every column of this rank's quotient rows
    double window_ms = 0;  // the window exchange, counted in EON_STAGE_EXCHANGE, not in the LDE
    const uint64_t next_step = 1ull << log_qd;
    const uint64_t block_rows = (q_rows + world - 1) / world;  // R: quotient rows per rank
    try {
        lde = pcs.get_evaluations_on_domain(trace_data, 0, quotient_domain);
        if (col_shard) {
            // rows of my columns -> columns of my rows: block h of `send` is the window of rank h
            auto x0 = tick();
            const uint64_t win_rows = block_rows + next_step;
            const uint64_t block_bytes = win_rows * slots * sizeof(eon_fr);
            DeviceBuffer send(block_bytes * world), recv(block_bytes * world);
            check(ctx, eon_shard_pack_rows_dev(ctx, lde.data(), q_rows, full_width, world, rank, next_step,
                                               send.as<eon_fr>()),
                  "pack window rows");
            check(ctx, eon_ctx_synchronize(ctx), "pack window rows");
            lde = DeviceMatrix();  // back to the buffer cache: the window is 1/world of it, plus 2^log_qd rows
            all_to_all(ctx, shard, send.get(), recv.get(), block_bytes);
            window = DeviceMatrix::alloc(win_rows, full_width);
            check(ctx, eon_shard_unpack_cols_dev(ctx, recv.as<eon_fr>(), q_rows, full_width, world, next_step,
                                                 window.mutable_data()),
                  "unpack window columns");
            window_ms = ms(x0, tick());
        }
        // recomputed each prove, as the reference does (prover.rs:321-322)
        if (pp) pre_lde = pcs.get_evaluations_on_domain(pp->data, 0, quotient_domain);
    } catch (...) {
        if (fs_thread.joinable()) fs_thread.join();
        throw;
    }
    if (fs_thread.joinable()) fs_thread.join();
    // check_constraints where the reference runs it (prover.rs:252-262): after generate_permutation,
    // before the permutation commitment and alpha.  The preprocessed trace is the caller's
    // (pre_trace of the lookup forms), else the evaluations the setup keeps.
    auto run_check = [&](const eon_fr* perm_trace, const std::vector<eon_fr>& ch) {
        const eon_fr* pre = lookups && lookups->pre_trace ? lookups->pre_trace
                            : pp                           ? pp->data.at(0).evals.data()
                                                           : nullptr;
        eon_constraint_report& r = constraint_check->report;
        check(ctx,
              eon_check_constraints_dev(ctx, air.prog, trace, pre, perm_trace, height, air.publics, air.n_public,
                                        ch.data(), n_challenges, nullptr, &r),
              "check_constraints");
        if (r.failures == 0) return;
        eon_air_program_stats stats{};
        (void)eon_air_program_info(air.prog, &stats);
        const Fr v = fr_mul(Fr::from_abi(r.value), Fr{{1, 0, 0, 0}});  // out of the Montgomery form
        char hex[2 + 64 + 1];
        std::snprintf(hex, sizeof(hex), "0x%016llx%016llx%016llx%016llx", (unsigned long long)v.l[3],
                      (unsigned long long)v.l[2], (unsigned long long)v.l[1], (unsigned long long)v.l[0]);
        throw Error(EON_E_CONSTRAINT, "Constraint failed at row " + std::to_string(r.row) + ": constraint " +
                                          std::to_string(r.constraint) + " of " +
                                          std::to_string(stats.num_constraints) + ", expected zero, got " + hex);
    };
    if (constraint_check && perm_width == 0) {
        run_check(nullptr, {});
        if (challenger) alpha = challenger->sample();  // prover.rs:300
    }
    if (perm_width > 0) {
        // generate_permutation (prover.rs:238-245), commit on the trace domain (:270), observe
        // (:273), alpha (:300), then the permutation trace on the quotient domain (:317-319)
        DeviceMatrix perm = DeviceMatrix::alloc(height, perm_width);
        std::vector<eon_fr> ch(n_challenges);
        for (uint32_t i = 0; i < n_challenges; i++) ch[i] = perm_challenges[i].abi();
        check(ctx,
              eon_lookup_permutation_dev(ctx, air.prog, trace, lookups->pre_trace, height, air.publics, air.n_public,
                                         ch.data(), n_challenges, perm.mutable_data()),
              "generate_permutation");
        if (constraint_check) run_check(perm.data(), ch);
        std::vector<std::pair<Domain, DeviceMatrix>> ev;
        ev.emplace_back(trace_domain, std::move(perm));
        pcs.commit(std::move(ev), perm_commit, perm_data);
        if (challenger) {
            challenger->observe_g1(perm_commit[0].data(), perm_commit[0].size());
            alpha = challenger->sample();
        }
        perm_lde = pcs.get_evaluations_on_domain(perm_data, 0, quotient_domain);
    }
    DeviceMatrix qv = col_shard ? DeviceMatrix() : DeviceMatrix::alloc(q_rows, 1);
    {
        t2 = tick();
        const eon_fr a = alpha.abi();
        if (col_shard) {
            // this rank's block of quotient rows, in a slot of R rows (the last ranks' may be short
            // or empty: the padding is zero and is trimmed after the all-gather)
            uint64_t row0 = 0, n_rows = 0;
            if (eon_shard_row_range(q_rows, world, rank, &row0, &n_rows) != EON_OK)
                throw Error(EON_E_ARG, "eon_shard_row_range");
            DeviceMatrix part = DeviceMatrix::alloc(block_rows, 1);
            if (n_rows < block_rows)
                hip_ok(hipMemsetAsync(part.mutable_data(), 0, block_rows * sizeof(eon_fr), st), "quotient block");
            check(ctx,
                  eon_quotient_values_rows_dev(ctx, air.prog, window.data(), log_n, log_qd, row0, n_rows, &a,
                                               air.publics, air.n_public, part.mutable_data()),
                  "quotient_values (rows)");
            qv = std::move(part);
        } else if (air.p2)
            check(ctx, eon_p2air_quotient_values_dev(ctx, air.p2, lde.data(), log_n, log_qd, &a, qv.mutable_data()),
                  "quotient_values");
        else if (perm_width > 0) {
            std::vector<eon_fr> ch(n_challenges);
            for (uint32_t i = 0; i < n_challenges; i++) ch[i] = perm_challenges[i].abi();
            check(ctx,
                  eon_quotient_values_lk_dev(ctx, air.prog, lde.data(), pp ? pre_lde.data() : nullptr, perm_lde.data(),
                                             log_n, log_qd, &a, air.publics, air.n_public, ch.data(), n_challenges,
                                             qv.mutable_data()),
                  "quotient_values");
        } else if (pp)
            check(ctx,
                  eon_quotient_values_pp_dev(ctx, air.prog, lde.data(), pre_lde.data(), log_n, log_qd, &a,
                                             air.publics, air.n_public, qv.mutable_data()),
                  "quotient_values");
        else
            check(ctx,
                  eon_quotient_values_dev(ctx, air.prog, lde.data(), log_n, log_qd, &a, air.publics, air.n_public,
                                          qv.mutable_data()),
                  "quotient_values");
    }
    check(ctx, eon_ctx_synchronize(ctx), "quotient_values");
    lde = DeviceMatrix();  // back to the buffer cache before the opening
    pre_lde = DeviceMatrix();
    perm_lde = DeviceMatrix();
    window = DeviceMatrix();
    auto t3 = tick();
    if (col_shard) {
        // the row blocks in rank order are the quotient itself: rank r's slot starts at row r R
        DeviceBuffer parts(sizeof(eon_fr) * block_rows * world);
        all_gather(ctx, shard, qv.data(), parts.get(), sizeof(eon_fr) * block_rows);
        qv = DeviceMatrix::alloc(q_rows, 1);
        hip_ok(hipMemcpyAsync(qv.mutable_data(), parts.get(), sizeof(eon_fr) * q_rows, hipMemcpyDeviceToDevice, st),
               "quotient blocks");
        (void)tick();
    } else if (shard) {
        DeviceBuffer parts(sizeof(eon_fr) * q_rows * world);
        all_gather(ctx, shard, qv.data(), parts.get(), sizeof(eon_fr) * q_rows);
        std::vector<eon_fr> w(world);
        for (uint32_t g = 0; g < world; g++)
            w[g] = fr_pow(alpha, (uint64_t)k_lane * (vector_len - (g + 1) * local_vl)).abi();
        check(ctx, eon_fr_lincomb_dev(ctx, parts.as<eon_fr>(), world, q_rows, w.data(), qv.mutable_data()),
              "combine partial quotients");
        (void)tick();
    }
    auto t3x = tick();
    // commit_quotient (prover.rs:371-372).  Sharded, chunk c is committed and opened by rank
    // c % world alone (commit/src/pcs.rs:82-101 commits the chunks independently) and the chunk
    // commitments are all-gathered before zeta; unsharded, every chunk here.
    std::vector<uint32_t> my_chunks;
    for (uint32_t c = rank; c < num_chunks; c += world) my_chunks.push_back(c);
    const uint32_t chunk_slots = (num_chunks + world - 1) / world;  // per rank, padded
    std::vector<std::vector<eon_g1_affine>> quotient_commit;
    std::vector<MatrixProverData> quotient_data;
    pcs.commit_quotient(quotient_domain, qv, num_chunks, quotient_commit, quotient_data, &my_chunks);
    std::vector<eon_g1_affine> chunk_commit(num_chunks);
    if (shard) {
        std::vector<eon_g1_affine> mine(chunk_slots, eon_g1_affine{});
        for (size_t i = 0; i < my_chunks.size(); i++) mine[i] = quotient_commit[i][0];
        const uint64_t bytes = chunk_slots * sizeof(eon_g1_affine);
        DeviceBuffer send(bytes), recv(bytes * world);
        hip_ok(hipMemcpyAsync(send.get(), mine.data(), bytes, hipMemcpyHostToDevice, st), "quotient commit");
        all_gather(ctx, shard, send.get(), recv.get(), bytes);
        std::vector<eon_g1_affine> all((uint64_t)chunk_slots * world);
        hip_ok(hipMemcpyAsync(all.data(), recv.get(), bytes * world, hipMemcpyDeviceToHost, st), "quotient commit");
        hip_ok(hipStreamSynchronize(st), "quotient commit");
        for (uint32_t c = 0; c < num_chunks; c++) chunk_commit[c] = all[(uint64_t)(c % world) * chunk_slots + c / world];
    } else {
        for (uint32_t c = 0; c < num_chunks; c++) chunk_commit[c] = quotient_commit[c][0];
    }
    Fr zeta = zeta_in;
    if (challenger) {
        for (const auto& q : chunk_commit) challenger->observe_g1(&q, 1);  // :373
        zeta = challenger->sample();                                        // :416
    }
    proof.alpha = alpha;
    proof.zeta = zeta;
    auto t4 = tick();
    const Fr zeta_next = trace_domain.next_point(zeta);  // prover.rs:416-419
    // the rounds in the reference's order (prover.rs:426-439): trace, permutation, quotient chunks,
    // preprocessed
    std::vector<OpenRound> rounds(1);
    rounds[0].data = &trace_data;
    rounds[0].points = {{zeta, zeta_next}};
    size_t i_perm = 0, i_pre = 0;
    if (perm_width > 0) {
        i_perm = rounds.size();
        rounds.emplace_back();
        rounds.back().data = &perm_data;
        rounds.back().points = {{zeta, zeta_next}};
    }
    const size_t i_quot = rounds.size();
    rounds.emplace_back();
    rounds.back().data = &quotient_data;
    rounds.back().points.assign(quotient_data.size(), std::vector<Fr>{zeta});
    if (pp) {  // round3 (prover.rs:431): after the quotient chunks
        i_pre = rounds.size();
        rounds.emplace_back();
        rounds.back().data = &pp->data;
        rounds.back().points = {{zeta, zeta_next}};
    }
    // the opening bases are the same on every rank: sharded over the process group
    // (eon_ctx_set_collective)
    struct CollectiveScope {
        eon_ctx* c;
        CollectiveScope(eon_ctx* c_, const eon_collective* s) : c(c_) {
            if (s) check(c, eon_ctx_set_collective(c, s), "eon_ctx_set_collective");
        }
        ~CollectiveScope() { (void)eon_ctx_set_collective(c, nullptr); }
    };
    std::vector<Opened> opened;
    if (batched) {
        // gamma follows the opened values, delta the witnesses (prover.h, BatchedOpening)
        Fr gamma = batched->gamma;
        if (challenger) {
            opened = pcs.open_values(rounds);
            for (const Opened& o : opened)
                for (const auto& mat : o.values)
                    for (const auto& at_point : mat)
                        for (const eon_fr& v : at_point) challenger->observe(Fr::from_abi(v));
            gamma = challenger->sample();
        }
        opened = pcs.open_batched(rounds, gamma, challenger ? &opened : nullptr);
        batched->gamma_used = gamma;
        if (challenger) {
            for (const Opened& o : opened)
                for (const auto& mat : o.witnesses)
                    for (const auto& at_point : mat) challenger->observe_g1(at_point.data(), at_point.size());
            batched->delta_used = challenger->sample();
        }
    } else {
        // The opening-bases collectives inside `open` are keyed by (height, point), in order of first
        // use.  The trace round comes first and every rank has at least one trace column (lanes; a
        // column range is never empty: world <= W), so every rank builds (N, zeta) and (N, zeta h)
        // -- the quotient chunks have N rows too and are opened at zeta, a key already there.  A
        // rank without a quotient chunk therefore issues exactly the collective calls of the others.
        CollectiveScope scope(ctx, shard);
        opened = pcs.open(rounds);  // prover.rs:424-442
    }
    auto t5 = tick();

    proof.quotient_commit = chunk_commit;
    proof.quotient_opened.resize(num_chunks);
    proof.quotient_witnesses.resize(num_chunks);
    if (!shard) {
        for (uint32_t c = 0; c < num_chunks; c++) {
            proof.quotient_opened[c] = opened[i_quot].values[c][0][0];
            proof.quotient_witnesses[c] = opened[i_quot].witnesses[c][0][0];
        }
    } else {
        // every rank's chunk openings to every rank: value (4 u64) | witness (8 u64) per slot
        constexpr uint32_t QREC = 12;
        std::vector<uint64_t> rec((uint64_t)chunk_slots * QREC, 0);
        for (size_t i = 0; i < my_chunks.size(); i++) {
            std::memcpy(&rec[i * QREC], &opened[i_quot].values[i][0][0], 32);
            std::memcpy(&rec[i * QREC + 4], &opened[i_quot].witnesses[i][0][0], 64);
        }
        const uint64_t bytes = rec.size() * sizeof(uint64_t);
        DeviceBuffer send(bytes), recv(bytes * world);
        hip_ok(hipMemcpyAsync(send.get(), rec.data(), bytes, hipMemcpyHostToDevice, st), "quotient openings");
        all_gather(ctx, shard, send.get(), recv.get(), bytes);
        std::vector<uint64_t> all(rec.size() * world);
        hip_ok(hipMemcpyAsync(all.data(), recv.get(), bytes * world, hipMemcpyDeviceToHost, st), "quotient openings");
        hip_ok(hipStreamSynchronize(st), "quotient openings");
        for (uint32_t c = 0; c < num_chunks; c++) {
            const uint64_t* r = &all[((uint64_t)(c % world) * chunk_slots + c / world) * QREC];
            std::memcpy(&proof.quotient_opened[c], r, 32);
            std::memcpy(&proof.quotient_witnesses[c], r + 4, 64);
        }
    }
    if (pp) {
        proof.pre_commit = pp->commitment;
        for (int p = 0; p < 2; p++) {
            proof.pre_opened[p] = opened[i_pre].values[0][p];
            proof.pre_witnesses[p] = opened[i_pre].witnesses[0][p];
        }
    }
    if (perm_width > 0) {
        proof.perm_challenges = perm_challenges;
        proof.perm_commit = perm_commit[0];
        for (int p = 0; p < 2; p++) {
            proof.perm_opened[p] = opened[i_perm].values[0][p];
            proof.perm_witnesses[p] = opened[i_perm].witnesses[0][p];
        }
    }
    const Opened& tr = opened[0];
    if (!shard) {
        proof.trace_commit = trace_commit[0];
        for (int p = 0; p < 2; p++) {
            proof.trace_opened[p] = tr.values[0][p];
            proof.trace_witnesses[p] = tr.witnesses[0][p];
        }
    } else {
        // every rank's columns land at their global positions (rank order = lane order)
        // (slots of `slots` columns: column ranges differ by one, the padding is zero)
        std::vector<uint64_t> rec((uint64_t)slots * RECORD, 0);
        for (uint32_t c = 0; c < width; c++) {
            uint64_t* r = rec.data() + (uint64_t)c * RECORD;
            std::memcpy(r, &trace_commit[0][c], 64);
            std::memcpy(r + 8, &tr.values[0][0][c], 32);
            std::memcpy(r + 12, &tr.values[0][1][c], 32);
            std::memcpy(r + 16, &tr.witnesses[0][0][c], 64);
            std::memcpy(r + 24, &tr.witnesses[0][1][c], 64);
        }
        const uint64_t bytes = rec.size() * sizeof(uint64_t);
        DeviceBuffer send(bytes), recv(bytes * world);
        hip_ok(hipMemcpyAsync(send.get(), rec.data(), bytes, hipMemcpyHostToDevice, st), "records");
        all_gather(ctx, shard, send.get(), recv.get(), bytes);
        std::vector<uint64_t> all(rec.size() * world);
        hip_ok(hipMemcpyAsync(all.data(), recv.get(), bytes * world, hipMemcpyDeviceToHost, st), "records");
        hip_ok(hipStreamSynchronize(st), "records");
        proof.trace_commit.resize(full_width);
        for (int p = 0; p < 2; p++) {
            proof.trace_opened[p].resize(full_width);
            proof.trace_witnesses[p].resize(full_width);
        }
        for (uint32_t g = 0; g < world; g++) {
            uint32_t c0, wl;
            cols_of(g, &c0, &wl);
            for (uint32_t k = 0; k < wl; k++) {
                const uint64_t* r = all.data() + ((uint64_t)g * slots + k) * RECORD;
                const uint64_t c = (uint64_t)c0 + k;
                std::memcpy(&proof.trace_commit[c], r, 64);
                std::memcpy(&proof.trace_opened[0][c], r + 8, 32);
                std::memcpy(&proof.trace_opened[1][c], r + 12, 32);
                std::memcpy(&proof.trace_witnesses[0][c], r + 16, 64);
                std::memcpy(&proof.trace_witnesses[1][c], r + 24, 64);
            }
        }
    }
    auto t6 = tick();
    proof.stage_ms[EON_STAGE_COMMIT_TRACE] = ms(t0, t1);
    proof.stage_ms[EON_STAGE_TRACE_LDE] = ms(t1, t2) - window_ms;
    proof.stage_ms[EON_STAGE_QUOTIENT] = ms(t2, t3);
    proof.stage_ms[EON_STAGE_EXCHANGE] = ms(t3, t3x) + window_ms;  // both data exchanges
    proof.stage_ms[EON_STAGE_COMMIT_QUOTIENT] = ms(t3x, t4);
    proof.stage_ms[EON_STAGE_OPEN] = ms(t4, t5);
    proof.stage_ms[EON_STAGE_ASSEMBLE] = ms(t5, t6);
    return proof;
}

}  // namespace eon_host
