// Evaluator::rotate_sum (not SEAL API) against rotate_vectors + add_inplace_reduced_error in order,
// word for word and scale for scale, on seeded keys at N = 2^13: a term list with a zero step, one
// with a step that has no key of its own (NAF: the one-by-one path) and one over mixed levels (the
// same); the sums of three FiberBatch fibers merged into one mhe_rotate_sum; an injected scratch
// allocation failure that must leave the destination's words alone.
//   rotate_sum_test
// and one sparse bootstrap_real_3 (N = 2^12, logn 10: trace_caller_test's boot mode) with the
// Bootstrapper's merged giant-step sums off and on: equal words and scale, mhe_rotsum_stats nonzero
// only in the second run.
//   rotate_sum_test boot
#include "mhe_boot.h"
#include "seal/seal.h"
#include "../../include/mhe.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

using namespace seal;

static int g_fail = 0;
static bool same(const Ciphertext &a, const Ciphertext &b)
{
    if (a.size() != b.size() || a.coeff_modulus_size() != b.coeff_modulus_size() || a.scale() != b.scale() ||
        a.parms_id() != b.parms_id())
        return false;
    const PolyStore &x = a.store(), &y = b.store();
    return x.words() == y.words() && std::memcmp(x.host(), y.host(), x.words() * 8) == 0;
}
static void check(const std::string &what, bool ok)
{
    std::printf("[%s] %s\n", ok ? "PASS" : "FAIL", what.c_str());
    if (!ok) g_fail++;
}
struct Stats
{
    std::uint64_t sums = 0, terms = 0;
};
static Stats rotsum_stats(const SEALContext &ctx, bool reset = false)
{
    Stats s;
    mhe_rotsum_stats(ctx.engine(), &s.sums, &s.terms, reset ? 1 : 0);
    return s;
}

static int run_sums()
{
    const int logN = 13;
    const std::size_t N = (std::size_t)1 << logN;
    std::vector<int> bits{ 51 };
    for (int i = 0; i < 6; i++) bits.push_back(46);
    bits.push_back(51);
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(N);
    parms.set_coeff_modulus(CoeffModulus::Create(N, bits));
    parms.set_random_generator(
        std::make_shared<Blake2xbPRNGFactory>(std::array<std::uint64_t, 8>{ 2, 7, 1, 8, 2, 8, 1, 8 }));
    SEALContext ctx(parms, true, sec_level_type::none);
    KeyGenerator keygen(ctx);
    PublicKey pk;
    keygen.create_public_key(pk);
    const int slots = (int)N / 2;
    // +-2^i for i < 5: step 3 below has no key of its own (SEAL's NAF path)
    std::vector<int> key_steps;
    for (int i = 0; i < 5; i++)
    {
        key_steps.push_back(1 << i);
        key_steps.push_back(slots - (1 << i));
    }
    GaloisKeys glk;
    keygen.create_galois_keys(key_steps, glk);
    CKKSEncoder encoder(ctx);
    Encryptor encryptor(ctx, pk);
    Evaluator ev(ctx, encoder);
    std::mt19937_64 g(12);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    // every term at its own scale: the sum must come out at the last term's
    auto fresh = [&](int drop, double scale) {
        std::vector<double> v(slots);
        for (auto &x : v) x = U(g);
        Plaintext p;
        Ciphertext c;
        encoder.encode(v, scale, p);
        encryptor.encrypt(p, c);
        for (int i = 0; i < drop; i++) ev.mod_switch_to_next_inplace(c);
        return c;
    };
    // the sequence rotate_sum replaces (Bootstrapper.cpp:1990-2015)
    auto one_by_one = [&](const std::vector<const Ciphertext *> &in, const std::vector<int> &st, Ciphertext &sum) {
        std::vector<Ciphertext> rot(in.size());
        std::vector<const Ciphertext *> rin;
        std::vector<int> rst;
        std::vector<Ciphertext *> rout;
        for (std::size_t i = 0; i < in.size(); i++)
            if (st[i] != 0)
            {
                rin.push_back(in[i]);
                rst.push_back(st[i]);
                rout.push_back(&rot[i]);
            }
        ev.rotate_vectors(rin, rst, glk, rout);
        Ciphertext acc;
        for (std::size_t i = 0; i < in.size(); i++)
        {
            const Ciphertext &term = st[i] != 0 ? rot[i] : *in[i];
            if (i == 0)
                acc = term;
            else
                ev.add_inplace_reduced_error(acc, term);
        }
        sum = std::move(acc);
    };
    auto ptrs = [](const std::vector<Ciphertext> &v) {
        std::vector<const Ciphertext *> p;
        for (const Ciphertext &c : v) p.push_back(&c);
        return p;
    };
    try
    {
        struct Case
        {
            const char *name;
            std::vector<int> steps;
            std::vector<int> drops;
            bool merged;
        };
        const std::vector<Case> cases{
            { "keyed steps", { 1, 2, slots - 4, 16, 8 }, { 1, 1, 1, 1, 1 }, true },
            { "a zero step in the middle", { slots - 2, 1, 0, 4, 16 }, { 3, 3, 3, 3, 3 }, true },
            { "a zero step first, ten terms", { 0, 1, 2, 4, 8, 16, slots - 1, slots - 2, slots - 4, slots - 8 },
              { 2, 2, 2, 2, 2, 2, 2, 2, 2, 2 }, true },
            { "a step without a key (NAF): one by one", { 1, 3, 2 }, { 0, 0, 0 }, false },
            { "mixed levels: one by one", { 1, 2, 4 }, { 0, 1, 0 }, false },
        };
        for (const Case &c : cases)
        {
            std::vector<Ciphertext> in;
            for (std::size_t i = 0; i < c.steps.size(); i++) in.push_back(fresh(c.drops[i], std::pow(2.0, 46) * (1.0 + 0.125 * i)));
            const std::vector<Ciphertext> keep = in;
            Ciphertext want, got;
            one_by_one(ptrs(in), c.steps, want);
            rotsum_stats(ctx, true);
            ev.rotate_sum(ptrs(in), c.steps, glk, got);
            const Stats s = rotsum_stats(ctx, true);
            // same(): words and scale; at equal levels the fold leaves the last term's scale
            bool ok = same(got, want) && (!c.merged || got.scale() == in.back().scale());
            for (std::size_t i = 0; i < in.size(); i++) ok = ok && same(in[i], keep[i]);
            std::size_t rotated = 0;
            for (int st : c.steps) rotated += st != 0;
            ok = ok && (c.merged ? (s.sums == 1 && s.terms == rotated) : (s.sums == 0 && s.terms == 0));
            check(std::string("rotate_sum == rotate_vectors + add_inplace_reduced_error: ") + c.name, ok);
        }
        {
            // the destination is one of the inputs
            std::vector<Ciphertext> in;
            for (int i = 0; i < 3; i++) in.push_back(fresh(1, std::pow(2.0, 46)));
            Ciphertext want;
            one_by_one(ptrs(in), { 1, 2, 4 }, want);
            ev.rotate_sum(ptrs(in), { 1, 2, 4 }, glk, in[1]);
            check("rotate_sum into one of its inputs", same(in[1], want));
        }
        {
            // three fibers, the same-numbered rotate_sum of each merged into one call
            const std::size_t M = 3;
            const std::vector<int> st{ 1, 0, slots - 2, 8 };
            std::vector<std::vector<Ciphertext>> in(M);
            for (auto &v : in)
                for (std::size_t i = 0; i < st.size(); i++) v.push_back(fresh(1, std::pow(2.0, 46)));
            std::vector<Ciphertext> alone(M), fibered(M);
            for (std::size_t m = 0; m < M; m++) ev.rotate_sum(ptrs(in[m]), st, glk, alone[m]);
            rotsum_stats(ctx, true);
            const std::uint64_t fb0 = merged_call_fallbacks();
            FiberBatch::run(M, [&](std::size_t m) { ev.rotate_sum(ptrs(in[m]), st, glk, fibered[m]); });
            const Stats s = rotsum_stats(ctx, true);
            bool ok = true;
            for (std::size_t m = 0; m < M; m++) ok = ok && same(fibered[m], alone[m]);
            std::printf("fibers: %zu member calls merged, %llu sums of %llu terms\n", FiberBatch::last_merged(),
                        (unsigned long long)s.sums, (unsigned long long)s.terms);
            check("FiberBatch (3 fibers): each fiber's rotate_sum == the same fiber alone", ok);
            check("FiberBatch: the three sums ran as one merged call", FiberBatch::last_merged() >= M && s.sums == M && s.terms == 3 * M);
            check("FiberBatch: no merged call fell back", merged_call_fallbacks() == fb0);
        }
        {
            // the first merged call at the top level (every one above ran lower): its accumulators have to
            // grow.  With that growth (nth 2) or the temporary before it (nth 1) failing, the call throws
            // and the destination keeps its words
            std::vector<Ciphertext> in;
            for (int i = 0; i < 3; i++) in.push_back(fresh(0, std::pow(2.0, 46)));
            const std::vector<int> st{ 1, 2, 4 };
            Ciphertext want;
            one_by_one(ptrs(in), st, want);
            bool ok = true;
            for (int nth = 1; nth <= 2; nth++)
            {
                Ciphertext dest = fresh(2, std::pow(2.0, 40));
                const Ciphertext before = dest;
                mhe_debug_fail_alloc(ctx.engine(), nth);
                bool threw = false;
                try
                {
                    ev.rotate_sum(ptrs(in), st, glk, dest);
                }
                catch (const std::exception &e)
                {
                    threw = true;
                    std::printf("  nth %d: %s\n", nth, e.what());
                }
                mhe_debug_fail_alloc(ctx.engine(), 0);
                ok = ok && threw && same(dest, before);
            }
            check("rotate_sum with a failing scratch allocation throws and leaves the destination's words", ok);
            Ciphertext dest = fresh(2, std::pow(2.0, 40));
            ev.rotate_sum(ptrs(in), st, glk, dest);
            check("rotate_sum after the failed calls == one by one", same(dest, want));
        }
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\n", e.what());
        g_fail++;
    }
    return g_fail;
}

// one sparse bootstrap, merged giant-step sums off and on (parameters: trace_caller_test's boot mode)
static int run_boot()
{
    const int logN = 12;
    const long logn = 10;
    const std::size_t N = (std::size_t)1 << logN;
    const long loge = 10, boundary_K = 25, boot_deg = 59, scale_factor = 2, inverse_deg = 1;
    const int logp = 46, logq = 51, remaining_level = 16, boot_level = 14, total_level = remaining_level + boot_level;
    std::vector<int> bits{ logq };
    for (int i = 0; i < remaining_level; i++) bits.push_back(logp);
    for (int i = 0; i < boot_level; i++) bits.push_back(logq);
    bits.push_back(51);
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(N);
    parms.set_coeff_modulus(CoeffModulus::Create(N, bits));
    parms.set_secret_key_hamming_weight(64);
    parms.set_random_generator(
        std::make_shared<Blake2xbPRNGFactory>(std::array<std::uint64_t, 8>{ 1, 2, 3, 4, 5, 6, 7, 8 }));
    SEALContext ctx(parms, true, sec_level_type::none);
    KeyGenerator keygen(ctx);
    PublicKey pk;
    keygen.create_public_key(pk);
    RelinKeys rlk;
    keygen.create_relin_keys(rlk);
    GaloisKeys glk;
    CKKSEncoder encoder(ctx);
    Encryptor encryptor(ctx, pk);
    Decryptor decryptor(ctx, keygen.secret_key());
    Evaluator evaluator(ctx, encoder);
    const double scale = std::pow(2.0, logp);
    Bootstrapper bt(loge, logn, logN - 1, total_level, scale, boundary_K, boot_deg, scale_factor, inverse_deg, ctx, keygen,
                    encoder, encryptor, decryptor, evaluator, rlk, glk);
    bt.prepare_mod_polynomial();
    std::vector<int> steps{ 0 };
    for (int i = 0; i < logN - 1; i++) steps.push_back(1 << i);
    bt.addLeftRotKeys_Linear_to_vector_3(steps);
    keygen.create_deferred_galois_keys(steps, glk);
    bt.slot_vec.push_back(logn);
    bt.generate_LT_coefficient_3();

    const long n = 1L << logn, Nh = (long)N / 2;
    std::mt19937_64 g(20261019);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<double> z(n), msg(Nh);
    for (auto &x : z) x = U(g);
    for (long i = 0; i < Nh; i++) msg[i] = z[i % n];
    Plaintext pt;
    encoder.encode(msg, scale, pt);
    Ciphertext ct;
    encryptor.encrypt(pt, ct);
    evaluator.mod_switch_to_inplace(ct, ctx.last_parms_id());
    try
    {
        Ciphertext out[2];
        Stats st[2];
        for (int on = 0; on < 2; on++)
        {
            Ciphertext in = ct;
            bt.set_merged_giant_sums(on != 0);
            rotsum_stats(ctx, true);
            bt.bootstrap_real_3(out[on], in);
            st[on] = rotsum_stats(ctx, true);
            std::printf("merged giant sums %s: %llu sums of %llu rotations\n", on ? "on" : "off",
                        (unsigned long long)st[on].sums, (unsigned long long)st[on].terms);
        }
        Plaintext dp;
        decryptor.decrypt(out[1], dp);
        std::vector<double> got;
        encoder.decode(dp, got);
        double err = 0;
        for (long i = 0; i < Nh; i++) err = std::max(err, std::fabs(got[i] - msg[i]));
        std::printf("bootstrap_real_3 (N 2^%d, logn %ld): max error %.3g\n", logN, logn, err);
        check("bootstrap with merged giant-step sums: the words and scale of the bootstrap without", same(out[0], out[1]));
        check("the bootstrap decrypts to its input", err < 1e-2);
        check("mhe_rotsum_stats: zero with the switch off, nonzero with it on",
              st[0].sums == 0 && st[0].terms == 0 && st[1].sums > 0 && st[1].terms > st[1].sums);
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\n", e.what());
        g_fail++;
    }
    return g_fail;
}

int main(int argc, char **argv)
{
    const int fails = (argc > 1 && std::string(argv[1]) == "boot") ? run_boot() : run_sums();
    std::printf(fails ? "%d FAILED\n" : "ALL PASSED\n", fails);
    return fails ? 1 : 0;
}
