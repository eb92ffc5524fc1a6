// Stand-alone host program for the verifier's prepare phase (plonky3_eon_amd/host/verify_prepare.*):
// prepare over 8 synthetic proofs of one synthetic program shape, once on one thread and once on 8
// threads (one proof each, as verify_many spreads them), under Fiat-Shamir and with given
// challenges.  The two runs must agree on everything prepare produces -- verdict, detail, the
// challenges, the opening lists, quotient(zeta), the staged rows -- and on every challenger's end
// state and next sample.  Meant to be built with -fsanitize=address,undefined and with
// -fsanitize=thread and run directly (tests/test_verify_prepare_host.py).  Prints "ok <verdicts>".
//
// The proofs are data, not proofs of anything: prepare checks no opening.  Per-column proofs carry
// arbitrary canonical coordinates; the batched ones, whose points prepare tests for membership in G1,
// carry the identity.  Proof 5 has a non-canonical opened value (batched: a verdict), proof 6 lacks
// its permutation part (a shape verdict), proof 7 has a trace degree above the pcs's.
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "verify_prepare.h"

using namespace eon_host;

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
eon_fr rand_fr() {  // top limb below 2^60: below both moduli
    eon_fr r;
    for (int i = 0; i < 4; i++) r.l[i] = next_u64();
    r.l[3] &= (1ull << 60) - 1;
    return r;
}
eon_g1_affine rand_point(bool identity) {
    eon_g1_affine p;
    std::memset(&p, 0, sizeof p);
    if (identity) return p;
    const eon_fr x = rand_fr(), y = rand_fr();
    for (int i = 0; i < 4; i++) p.x[i] = x.l[i], p.y[i] = y.l[i];
    return p;
}

constexpr ProgShape SHAPE{5, 2, 2, 2, 3, 1};  // width, publics, preprocessed, permutation, challenges, log_qd
constexpr uint32_t CHUNKS = 2;
constexpr uint64_t MAX_DEGREE = 255;

struct Synthetic {
    std::vector<eon_g1_affine> tc, qc, tw, qw, pw, mc, mw, vk;
    std::vector<eon_fr> to, qo, po, mo, publics, challenges;
    eon_proof_lk lk;
    VerifyInputs in;
};

void make(Synthetic& s, int kind) {
    const bool batched = kind == 4 || kind == 5;
    const uint32_t w = SHAPE.width, pw = SHAPE.pre_width, mw = SHAPE.perm_width;
    auto points = [&](std::vector<eon_g1_affine>& v, size_t n) {
        for (size_t i = 0; i < n; i++) v.push_back(rand_point(batched));
    };
    auto values = [&](std::vector<eon_fr>& v, size_t n) {
        for (size_t i = 0; i < n; i++) v.push_back(rand_fr());
    };
    points(s.tc, w), points(s.qc, CHUNKS), points(s.mc, mw), points(s.vk, pw);
    points(s.tw, batched ? 2 : 2 * w), points(s.qw, CHUNKS), points(s.pw, batched ? 2 : 2 * pw);
    points(s.mw, batched ? 2 : 2 * mw);
    values(s.to, 2 * w), values(s.qo, CHUNKS), values(s.po, 2 * pw), values(s.mo, 2 * mw);
    values(s.publics, SHAPE.n_public), values(s.challenges, SHAPE.n_challenges);
    if (kind == 5) s.to[3].l[3] = ~0ull;  // not a canonical Fr
    std::memset(&s.lk, 0, sizeof s.lk);
    eon_proof& b = s.lk.pp.base;
    b.trace_commit = s.tc.data(), b.quotient_commit = s.qc.data();
    b.trace_opened = s.to.data(), b.trace_witnesses = s.tw.data();
    b.quotient_opened = s.qo.data(), b.quotient_witnesses = s.qw.data();
    b.degree_bits = kind == 7 ? 9 : 3 + kind % 2;
    s.lk.pp.preprocessed_opened = s.po.data(), s.lk.pp.preprocessed_witnesses = s.pw.data();
    if (kind != 6) {
        s.lk.permutation_commit = s.mc.data();
        s.lk.permutation_opened = s.mo.data(), s.lk.permutation_witnesses = s.mw.data();
    }
    VerifyInputs& in = s.in;
    in.proof = &s.lk;
    in.publics = s.publics.data(), in.n_public = SHAPE.n_public;
    in.vk_width = pw, in.vk_degree_bits = b.degree_bits, in.vk_commitment = s.vk.data();
    in.challenges = s.challenges.data(), in.n_challenges = SHAPE.n_challenges;
    in.alpha = Fr::from_abi(rand_fr()), in.zeta = Fr::from_abi(rand_fr());
    in.batched = batched;
    in.gamma = Fr::from_abi(rand_fr()), in.delta = Fr::from_abi(rand_fr());
}

template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
bool same_fr(const std::vector<Fr>& a, const std::vector<Fr>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!(a[i] == b[i])) return false;
    return true;
}

bool same(const Prepared& a, const Prepared& b) {
    return a.done == b.done && a.out.verdict == b.out.verdict && a.out.detail == b.out.detail &&
           a.out.alpha == b.out.alpha && a.out.zeta == b.out.zeta && a.out.gamma == b.out.gamma &&
           a.out.delta == b.out.delta && same_fr(a.out.challenges, b.out.challenges) && a.log_n == b.log_n &&
           a.pre_width == b.pre_width && a.batched == b.batched && a.quotient == b.quotient &&
           a.zeta_on_domain == b.zeta_on_domain && same_bytes(a.cs, b.cs) && same_bytes(a.ws, b.ws) &&
           same_bytes(a.vs, b.vs) && same_bytes(a.zs, b.zs) && same_bytes(a.pts, b.pts) &&
           same_bytes(a.scal, b.scal) && same_bytes(a.rows, b.rows);
}

struct Run {
    std::vector<Prepared> prepared;
    std::vector<DuplexChallenger> challengers;
};

// thread t of `threads` prepares proofs t, t + threads, ...: verify_many's split
Run run(const std::vector<Synthetic>& proofs, const Poseidon2Bn254& perm, bool fs, size_t threads) {
    Run r;
    const size_t n = proofs.size();
    r.prepared.resize(n);
    r.challengers.assign(n, DuplexChallenger(perm));
    const eon_air_program* prog = reinterpret_cast<const eon_air_program*>(&SHAPE);  // only tested for null
    auto work = [&](size_t t) {
        for (size_t i = t; i < n; i += threads) {
            VerifyInputs in = proofs[i].in;
            in.prog = prog;
            r.prepared[i] = prepare(MAX_DEGREE, SHAPE, in, fs ? &r.challengers[i] : nullptr);
        }
    };
    if (threads == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (size_t t = 0; t < threads; t++) pool.emplace_back(work, t);
        for (std::thread& th : pool) th.join();
    }
    return r;
}

}  // namespace

int main() {
    std::vector<eon_fr> begin(4 * 3), partial(22), end(4 * 3);
    for (auto* v : {&begin, &partial, &end})
        for (eon_fr& x : *v) x = rand_fr();
    const eon_poseidon2_constants consts{4, 22, begin.data(), partial.data(), end.data()};
    const Poseidon2Bn254 perm(consts);
    std::vector<Synthetic> proofs(8);
    for (int k = 0; k < 8; k++) make(proofs[k], k);
    std::string verdicts;
    for (const bool fs : {true, false}) {
        Run one = run(proofs, perm, fs, 1), many = run(proofs, perm, fs, 8);
        for (size_t i = 0; i < proofs.size(); i++) {
            if (!same(one.prepared[i], many.prepared[i])) {
                std::printf("proof %zu (%s): prepare differs between 1 and 8 threads\n", i, fs ? "fs" : "given");
                return 1;
            }
            for (int k = 0; k < DuplexChallenger::WIDTH; k++)
                if (!(one.challengers[i].state()[k] == many.challengers[i].state()[k])) {
                    std::printf("proof %zu: challenger state differs\n", i);
                    return 1;
                }
            if (!(one.challengers[i].sample() == many.challengers[i].sample())) {
                std::printf("proof %zu: the challengers' next samples differ\n", i);
                return 1;
            }
            verdicts += std::to_string(one.prepared[i].out.verdict);
        }
        // distinct proofs give distinct challenges: a challenger shared by two threads would show
        for (size_t i = 0; fs && i < proofs.size(); i++)
            for (size_t j = 0; j < i; j++)
                if (!one.prepared[i].done && !one.prepared[j].done &&
                    one.prepared[i].out.zeta == one.prepared[j].out.zeta) {
                    std::printf("proofs %zu and %zu sampled the same zeta\n", j, i);
                    return 1;
                }
        verdicts += fs ? " " : "";
    }
    std::printf("ok %s\n", verdicts.c_str());
    return 0;
}
