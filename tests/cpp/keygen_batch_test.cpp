// Key generation through one mhe_encrypt_sk_batch per key (batched launches on) against the per-digit
// sequence of general-purpose calls (batched launches off), word for word, at N = 2^13 on two contexts
// whose factories are the same seed sequence: the public key, the relinearization key,
// create_galois_keys({1, 2, -1}), truncated keys of 1, 2 and K-1 digits, a deferred key grown from
// level 2 to level 4; the seeded serializations byte for byte and a seeded save -> load round trip;
// mhe_keygen_stats (entries = the digits made, no overflow); a rotation and a relinearization with
// the batched keys decrypt correctly.  Then the overflow side, on a chain of 60-bit primes just above
// 1.5 * 2^59 (one uniform word in 64 is redrawn): with the redraw buffer limited to 8 words
// (mhe_debug_keygen_cap) every batched key overflows and is redone from its seeds, and equals the
// sequence's, as do the unlimited batched keys with their redraws on the device.
//   keygen_batch_test
#include "seal/seal.h"
#include "../../include/mhe.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>

using namespace seal;

static int g_fail = 0;
static void check(const std::string &what, bool ok)
{
    std::printf("[%s] %s\n", ok ? "PASS" : "FAIL", what.c_str());
    if (!ok) g_fail++;
}
static bool same(const PolyStore &x, const PolyStore &y)
{
    return x.words() == y.words() && x.words() && std::memcmp(x.host(), y.host(), x.words() * 8) == 0;
}
static bool same_keys(const KSwitchKeys &a, const KSwitchKeys &b, const std::vector<std::size_t> &indices)
{
    bool ok = true;
    for (std::size_t i : indices)
        ok = ok && a.has_index(i) && b.has_index(i) && a.limbs_of(i) == b.limbs_of(i) && same(a.key(i), b.key(i));
    return ok;
}

constexpr std::size_t N = (std::size_t)1 << 13;
constexpr int LOG_N = 13;

// One side of the comparison: side 0 runs with batched launches off, side 1 with them on.
struct Side
{
    bool batched;
    SEALContext ctx;
    std::unique_ptr<KeyGenerator> kg;
    static EncryptionParameters parms(std::shared_ptr<UniformRandomGeneratorFactory> f, std::vector<Modulus> cm)
    {
        EncryptionParameters p(scheme_type::ckks);
        p.set_poly_modulus_degree(N);
        p.set_coeff_modulus(cm.empty() ? CoeffModulus::Create(N, { 51, 46, 46, 46, 51 }) : cm);
        p.set_random_generator(std::move(f));
        return p;
    }
    Side(bool on, std::shared_ptr<UniformRandomGeneratorFactory> f, std::vector<Modulus> cm = {})
        : batched(on), ctx(parms(std::move(f), std::move(cm)), true, sec_level_type::none)
    {
        kg = std::make_unique<KeyGenerator>(ctx);
    }
    template <class F>
    void run(F &&f)
    {
        set_batched_launches(batched);
        f(*this);
        set_batched_launches(true);
    }
};

struct Stats
{
    std::uint64_t entries, groups, redrawn, overflows;
};
static Stats stats(const Side &s)
{
    Stats v{};
    if (mhe_keygen_stats(s.ctx.engine(), &v.entries, &v.groups, &v.redrawn, &v.overflows, 0) != 0) g_fail++;
    return v;
}

// Miller-Rabin with the first 12 primes as bases: deterministic below 2^64
static std::uint64_t mulmod(std::uint64_t a, std::uint64_t b, std::uint64_t m)
{
    return (std::uint64_t)((unsigned __int128)a * b % m);
}
static std::uint64_t powmod(std::uint64_t a, std::uint64_t e, std::uint64_t m)
{
    std::uint64_t r = 1;
    for (; e; e >>= 1, a = mulmod(a, a, m))
        if (e & 1) r = mulmod(r, a, m);
    return r;
}
static bool is_prime(std::uint64_t q)
{
    std::uint64_t d = q - 1;
    int s = 0;
    for (; !(d & 1); d >>= 1) s++;
    for (std::uint64_t a : { 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37 })
    {
        std::uint64_t x = powmod(a, d, q);
        if (x == 1 || x == q - 1) continue;
        bool composite = true;
        for (int i = 1; i < s && composite; i++)
        {
            x = mulmod(x, x, q);
            composite = x != q - 1;
        }
        if (composite) return false;
    }
    return true;
}
// NTT primes just above 1.5 * 2^59: 2^64 mod q ~ q / 3, so a word is redrawn with probability 1/64
static std::vector<Modulus> heavy_chain(std::size_t count)
{
    std::vector<Modulus> cm;
    for (std::uint64_t q = (3ull << 58) + 1; cm.size() < count; q += 2 * N)
        if (is_prime(q)) cm.push_back(Modulus(q));
    return cm;
}

// The overflow side: sequence, batched, and batched with the redraw buffer limited to 8 words.
static void overflow_side()
{
    const prng_seed_type seed = { 8, 7, 6, 5, 4, 3, 2, 1 };
    const std::vector<Modulus> cm = heavy_chain(5);
    Side off(false, std::make_shared<Blake2xbSeedSequence>(seed), cm), on(true, std::make_shared<Blake2xbSeedSequence>(seed), cm),
        capped(true, std::make_shared<Blake2xbSeedSequence>(seed), cm);
    if (mhe_debug_keygen_cap(capped.ctx.engine(), 8) != 0) g_fail++;
    Side *sides[3] = { &off, &on, &capped };
    const std::size_t K = on.ctx.key_size();
    const std::uint32_t elt = mhe_galois_elt_from_step(LOG_N, 1);
    const std::size_t gi = GaloisKeys::get_index(elt), ri = RelinKeys::get_index(2);
    PublicKey pk[3];
    RelinKeys rk[3], rl[3];
    GaloisKeys gk[3], tk[3], dk[3];
    Ciphertext rot[3];
    std::vector<double> v(N / 2);
    for (std::size_t j = 0; j < v.size(); j++) v[j] = std::cos(0.002 * (double)j);
    for (int i = 0; i < 3; i++)
        sides[i]->run([&](Side &s) {
            s.kg->create_public_key(pk[i]);
            s.kg->create_relin_keys(rk[i]);
            s.kg->create_galois_keys(std::vector<int>{ 1 }, gk[i]);
            s.kg->create_galois_keys(std::vector<std::pair<std::uint32_t, std::size_t>>{ { elt, 2 } }, tk[i]);
            std::ostringstream b;
            s.kg->create_relin_keys().save(b);
            std::istringstream in(b.str());
            rl[i].load(s.ctx, in); // the expansion of saved seeds: rnd::sample_uniform_dev and its redo
            CKKSEncoder encoder(s.ctx);
            Encryptor enc(s.ctx, pk[i]);
            Evaluator ev(s.ctx, encoder);
            s.kg->create_deferred_galois_keys({ 1 }, dk[i]);
            Plaintext p;
            Ciphertext c;
            encoder.encode(v, std::pow(2.0, 40), p);
            enc.encrypt(p, c);
            ev.rotate_vector(c, 1, dk[i], rot[i]); // the deferred provider materialises (and redoes) its key
        });
    const Stats a = stats(off), b = stats(on), c = stats(capped);
    std::printf("  heavy chain: batched %llu redrawn, %llu overflows; limited to 8 words %llu redrawn, %llu overflows\n",
                (unsigned long long)b.redrawn, (unsigned long long)b.overflows, (unsigned long long)c.redrawn,
                (unsigned long long)c.overflows);
    check("heavy chain: the batched side redrew words on the device and never overflowed", b.redrawn > 1000 && b.overflows == 0);
    check("heavy chain: the sequence side never used the device redraw", a.entries == 0 && a.redrawn == 0);
    // one entry per digit and public key, each rejecting about 5 * 128 words against 8
    check("limited buffer: every batched entry overflowed", c.entries > 0 && c.overflows >= c.entries);
    for (int i = 1; i < 3; i++)
    {
        const std::string who = i == 1 ? "heavy chain, batched" : "limited buffer, redone";
        check(who + ": public key == sequence", same(pk[0].data().store(), pk[i].data().store()));
        check(who + ": relinearization key == sequence", same_keys(rk[0], rk[i], { ri }));
        check(who + ": Galois key == sequence", same_keys(gk[0], gk[i], { gi }));
        check(who + ": truncated key == sequence", same_keys(tk[0], tk[i], { gi }) && tk[i].limbs_of(gi) == 3);
        check(who + ": seeded save -> load == sequence", same_keys(rl[0], rl[i], { ri }));
        check(who + ": deferred key == sequence", same_keys(dk[0], dk[i], { gi }) && dk[i].limbs_of(gi) == K);
        check(who + ": rotation with it == sequence", same(rot[0].store(), rot[i].store()));
    }
}

int main()
{
    const prng_seed_type seed = { 1, 2, 3, 4, 5, 6, 7, 8 };
    try
    {
        Side off(false, std::make_shared<Blake2xbSeedSequence>(seed)), on(true, std::make_shared<Blake2xbSeedSequence>(seed));
        Side *sides[2] = { &off, &on };
        const std::size_t K = on.ctx.key_size();
        std::uint64_t digits_made = 0;
        check("both sides drew the same secret key",
              same(off.kg->secret_key().data().store(), on.kg->secret_key().data().store()));

        PublicKey pk[2];
        RelinKeys rk[2];
        GaloisKeys gk[2], tk[2], dk[2];
        std::string pk_bytes[2], rk_bytes[2], gk_bytes[2];
        const std::vector<int> steps = { 1, 2, -1 };
        std::vector<std::uint32_t> elts;
        std::vector<std::size_t> gidx;
        for (int st : steps)
        {
            elts.push_back(mhe_galois_elt_from_step(LOG_N, st));
            gidx.push_back(GaloisKeys::get_index(elts.back()));
        }
        // truncated keys: the ciphertext levels 1, 2 and K-1 give 1, 2 and K-1 digits
        const std::vector<std::pair<std::uint32_t, std::size_t>> trunc = { { elts[0], 1 }, { elts[1], 2 }, { elts[2], K - 1 } };
        for (int i = 0; i < 2; i++)
            sides[i]->run([&](Side &s) {
                s.kg->create_public_key(pk[i]);
                s.kg->create_relin_keys(rk[i]);
                s.kg->create_galois_keys(steps, gk[i]);
                s.kg->create_galois_keys(trunc, tk[i]);
                std::ostringstream a, b, c;
                s.kg->create_public_key().save(a);
                s.kg->create_relin_keys().save(b);
                s.kg->create_galois_keys(steps).save(c);
                pk_bytes[i] = a.str();
                rk_bytes[i] = b.str();
                gk_bytes[i] = c.str();
            });
        digits_made += 2 * (1 + (K - 1) + 3 * (K - 1)) + (1 + 2 + (K - 1));
        check("public key: batched == sequence", same(pk[0].data().store(), pk[1].data().store()));
        check("relinearization key: batched == sequence", same_keys(rk[0], rk[1], { RelinKeys::get_index(2) }));
        check("create_galois_keys({1, 2, -1}): batched == sequence", same_keys(gk[0], gk[1], gidx));
        check("truncated keys of 1, 2 and K-1 digits: batched == sequence", same_keys(tk[0], tk[1], gidx));
        check("truncated keys store digits + 1 limbs",
              tk[1].limbs_of(gidx[0]) == 2 && tk[1].limbs_of(gidx[1]) == 3 && tk[1].limbs_of(gidx[2]) == K);
        check("seeded public key serializations are equal (the seeds too)", pk_bytes[0] == pk_bytes[1] && !pk_bytes[0].empty());
        check("seeded relinearization key serializations are equal", rk_bytes[0] == rk_bytes[1] && !rk_bytes[0].empty());
        check("seeded Galois key serializations are equal", gk_bytes[0] == gk_bytes[1] && !gk_bytes[0].empty());

        // seeded save -> load: the expansion of the saved seeds (the device uniform sampler) gives the
        // same key on both sides
        RelinKeys rl[2];
        GaloisKeys gl[2];
        for (int i = 0; i < 2; i++)
            sides[i]->run([&](Side &s) {
                std::istringstream b(rk_bytes[i]), c(gk_bytes[i]);
                rl[i].load(s.ctx, b);
                gl[i].load(s.ctx, c);
            });
        check("seeded save -> load of the relinearization key: batched == sequence",
              same_keys(rl[0], rl[1], { RelinKeys::get_index(2) }));
        check("seeded save -> load of the Galois keys: batched == sequence", same_keys(gl[0], gl[1], gidx));

        // a deferred key materialised at level 2 and grown to level 4 by the rotations that need it
        const double scale = std::pow(2.0, 40);
        std::vector<double> v(N / 2);
        for (std::size_t j = 0; j < v.size(); j++) v[j] = std::sin(0.001 * (double)j);
        Ciphertext rot2[2], rot4[2], relin[2];
        for (int i = 0; i < 2; i++)
            sides[i]->run([&](Side &s) {
                CKKSEncoder encoder(s.ctx);
                Encryptor enc(s.ctx, pk[i]);
                Evaluator ev(s.ctx, encoder);
                s.kg->create_deferred_galois_keys({ 1 }, dk[i]);
                Plaintext p;
                Ciphertext c4, c2;
                encoder.encode(v, scale, p);
                enc.encrypt(p, c4);
                c2 = c4;
                ev.mod_switch_to_next_inplace(c2);
                ev.mod_switch_to_next_inplace(c2);
                ev.rotate_vector(c2, 1, dk[i], rot2[i]);
                ev.rotate_vector(c4, 1, dk[i], rot4[i]);
                ev.multiply(c4, c4, relin[i]);
                ev.relinearize_inplace(relin[i], rk[i]);
                ev.rescale_to_next_inplace(relin[i]);
            });
        digits_made += 2 + (K - 1);
        check("deferred key grown from level 2 to level 4: batched == sequence", same_keys(dk[0], dk[1], { gidx[0] }));
        check("the deferred key holds K limbs after the growth", dk[1].limbs_of(gidx[0]) == K);
        check("rotations with it: batched == sequence",
              same(rot2[0].store(), rot2[1].store()) && same(rot4[0].store(), rot4[1].store()));

        // a rotation and a relinearization with the batched keys decrypt correctly
        {
            CKKSEncoder encoder(on.ctx);
            Decryptor dec(on.ctx, on.kg->secret_key());
            Plaintext p;
            std::vector<double> r, m;
            dec.decrypt(rot4[1], p);
            encoder.decode(p, r);
            dec.decrypt(relin[1], p);
            encoder.decode(p, m);
            double er = 0, em = 0;
            for (std::size_t j = 0; j < v.size(); j++)
            {
                er = std::max(er, std::fabs(r[j] - v[(j + 1) % v.size()]));
                em = std::max(em, std::fabs(m[j] - v[j] * v[j]));
            }
            std::printf("  rotation error %.3g, relinearization error %.3g\n", er, em);
            // Worst case of a key switch: each of the K-1 digits adds at most n (q_j / 2) 21 / P <= 21 n to
            // a coefficient (|e| <= 21, q_j <= 2P) and a slot sums n coefficients, so 4 * 21 n^2 / 2^40 =
            // 5.2e-3 at n = 2^13; the fresh encryption's and the rescale's noise are far below that.  A wrong
            // key leaves values of the size of q / scale.
            check("a rotation with a batched key decrypts", er < 1e-2);
            check("a relinearization with a batched key decrypts", em < 1e-2);
        }

        const Stats a = stats(off), b = stats(on);
        std::printf("  batched side: %llu entries in %llu groups, %llu redrawn, %llu overflows\n",
                    (unsigned long long)b.entries, (unsigned long long)b.groups, (unsigned long long)b.redrawn,
                    (unsigned long long)b.overflows);
        check("the sequence side never took the batch path", a.entries == 0 && a.groups == 0);
        check("the batched side made every digit (and public key) by the batch path", b.entries == digits_made);
        check("no overflow", a.overflows == 0 && b.overflows == 0);
        overflow_side();
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\n", e.what());
        g_fail++;
    }
    if (g_fail)
        std::printf("%d FAILED\n", g_fail);
    else
        std::printf("ALL PASSED\n");
    return g_fail ? 1 : 0;
}
