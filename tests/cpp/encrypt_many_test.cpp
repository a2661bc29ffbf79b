// Encryptor::encrypt_many / encrypt_zero_many (not SEAL API) against the same sequence of encrypt /
// encrypt_zero calls, word for word with scales and parms_ids, at N = 2^13: two encryptors on
// identically seeded contexts, batches of 1, 3 and 9 (a full round of 8 and a remainder) at the first
// and the second level, the same with batched launches off, the exceptions (each leaving every
// destination as it was).
//   encrypt_many_test
#include "seal/seal.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>

using namespace seal;

static int g_fail = 0;
static void check(const std::string &what, bool ok)
{
    std::printf("[%s] %s\n", ok ? "PASS" : "FAIL", what.c_str());
    if (!ok) g_fail++;
}
static bool same(const Ciphertext &a, const Ciphertext &b)
{
    if (a.size() != b.size() || a.coeff_modulus_size() != b.coeff_modulus_size() || a.scale() != b.scale() ||
        a.parms_id() != b.parms_id() || a.is_ntt_form() != b.is_ntt_form())
        return false;
    const PolyStore &x = a.store(), &y = b.store();
    return x.words() == y.words() && std::memcmp(x.host(), y.host(), x.words() * 8) == 0;
}
static bool all_same(const std::vector<Ciphertext> &a, const std::vector<Ciphertext> &b)
{
    bool ok = a.size() == b.size();
    for (std::size_t i = 0; ok && i < a.size(); i++) ok = same(a[i], b[i]);
    return ok;
}
static std::vector<Ciphertext *> mptrs(std::vector<Ciphertext> &v)
{
    std::vector<Ciphertext *> p;
    for (Ciphertext &x : v) p.push_back(&x);
    return p;
}
static std::vector<const Plaintext *> first(const std::vector<Plaintext> &v, std::size_t count)
{
    std::vector<const Plaintext *> p;
    for (std::size_t i = 0; i < count; i++) p.push_back(&v[i]);
    return p;
}

// One side of the comparison: a context whose factory is seeded with {1..8}, its keys and encryptor.
struct Side
{
    SEALContext ctx;
    PublicKey pk;
    SecretKey sk;
    std::unique_ptr<Encryptor> enc;
    static EncryptionParameters parms(std::shared_ptr<UniformRandomGeneratorFactory> f)
    {
        const std::size_t N = (std::size_t)1 << 13;
        EncryptionParameters p(scheme_type::ckks);
        p.set_poly_modulus_degree(N);
        p.set_coeff_modulus(CoeffModulus::Create(N, { 51, 46, 46, 51 }));
        p.set_random_generator(std::move(f));
        return p;
    }
    explicit Side(std::shared_ptr<UniformRandomGeneratorFactory> f) : ctx(parms(std::move(f)), true, sec_level_type::none)
    {
        KeyGenerator keygen(ctx);
        keygen.create_public_key(pk);
        sk = keygen.secret_key();
        enc = std::make_unique<Encryptor>(ctx, pk);
    }
};

// runs f, expecting exception E with text `text`
template <class E, class F>
static bool throws(const std::string &text, F &&f)
{
    try
    {
        f();
    }
    catch (const E &e)
    {
        std::printf("  %s\n", e.what());
        return text == e.what();
    }
    catch (const std::exception &e)
    {
        std::printf("  other exception: %s\n", e.what());
    }
    return false;
}

// pts / ptsb: the same plaintexts, encoded on each side's own context (and stream)
static void compare(const std::string &name, Side &a, Side &b, const std::vector<Plaintext> &pts,
                    const std::vector<Plaintext> &ptsb, parms_id_type id)
{
    for (std::size_t count : { (std::size_t)1, (std::size_t)3, (std::size_t)9 })
    {
        // side a: the single calls; side b: one batch.  Both factories have issued the same seeds so far.
        std::vector<Ciphertext> want(count), got(count), wantz(count), gotz(count);
        for (std::size_t i = 0; i < count; i++) a.enc->encrypt(pts[i], want[i]);
        b.enc->encrypt_many(first(ptsb, count), mptrs(got));
        check(name + ": encrypt_many of " + std::to_string(count) + " == the encrypt sequence", all_same(got, want));
        bool meta = true;
        for (std::size_t i = 0; i < count; i++) meta = meta && got[i].scale() == pts[i].scale() && got[i].parms_id() == id;
        check(name + ": scales and parms_ids are the plaintexts'", meta);
        for (std::size_t i = 0; i < count; i++) a.enc->encrypt_zero(id, wantz[i]);
        b.enc->encrypt_zero_many(id, mptrs(gotz));
        check(name + ": encrypt_zero_many of " + std::to_string(count) + " == the encrypt_zero sequence",
              all_same(gotz, wantz));
    }
}

int main()
{
    const prng_seed_type seed = { 1, 2, 3, 4, 5, 6, 7, 8 };
    const double scale = std::pow(2.0, 40);
    try
    {
        for (int sequence = 0; sequence <= 1; sequence++)
        {
            // Blake2xbPRNGFactory hands every generator the seed itself; Blake2xbSeedSequence a new seed
            // per generator, so there the order of the draws shows in the words
            auto factory = [&]() -> std::shared_ptr<UniformRandomGeneratorFactory> {
                if (sequence) return std::make_shared<Blake2xbSeedSequence>(seed);
                return std::make_shared<Blake2xbPRNGFactory>(seed);
            };
            const std::string fname = sequence ? "seed sequence" : "fixed seed";
            Side a(factory()), b(factory());
            check(fname + ": both sides made the same public key",
                  std::memcmp(a.pk.data().store().host(), b.pk.data().store().host(), a.pk.data().store().words() * 8) == 0);
            CKKSEncoder encoder(a.ctx), encoder_b(b.ctx);
            const std::size_t slots = encoder.slot_count();
            const parms_id_type id0 = a.ctx.first_parms_id(),
                                id1 = a.ctx.first_context_data()->next_context_data()->parms_id();
            std::mt19937_64 g(7);
            std::uniform_real_distribution<double> U(-1.0, 1.0);
            std::vector<Plaintext> p0(9), p1(9), q0(9), q1(9);
            for (std::size_t i = 0; i < 9; i++)
            {
                std::vector<double> v(slots);
                for (double &x : v) x = U(g);
                encoder.encode(v, id0, scale * (double)(i + 1), p0[i]);
                encoder.encode(v, id1, scale, p1[i]);
                encoder_b.encode(v, id0, scale * (double)(i + 1), q0[i]);
                encoder_b.encode(v, id1, scale, q1[i]);
            }
            for (int batched = 1; batched >= 0; batched--)
            {
                set_batched_launches(batched != 0);
                const std::string how = fname + (batched ? ", batched launches" : ", batched launches off");
                compare(how + ", first level", a, b, p0, q0, id0);
                compare(how + ", second level", a, b, p1, q1, id1);
            }
            set_batched_launches(true);
            if (sequence) continue;
            // the exceptions: every destination keeps its words
            std::vector<Ciphertext> keep(3), dest(3);
            for (std::size_t i = 0; i < 3; i++) a.enc->encrypt(p0[i], keep[i]);
            for (int batched = 1; batched >= 0; batched--)
            {
                set_batched_launches(batched != 0);
                const std::string how = batched ? " (batched launches)" : " (batched launches off)";
                dest = keep;
                std::vector<Plaintext> bad(p0.begin(), p0.begin() + 3);
                bad[1].parms_id() = parms_id_zero;
                check("a plaintext not in NTT form throws" + how,
                      throws<std::invalid_argument>("plain must be in NTT form",
                                                    [&] { a.enc->encrypt_many(first(bad, 3), mptrs(dest)); }));
                check("and every destination keeps its words" + how, all_same(dest, keep));
                bad[1].parms_id() = parms_id_type{ 1, 2, 3, 4 };
                check("a plaintext of unknown parameters throws" + how,
                      throws<std::invalid_argument>("plain is not valid for encryption parameters",
                                                    [&] { a.enc->encrypt_many(first(bad, 3), mptrs(dest)); }));
                check("and every destination keeps its words" + how, all_same(dest, keep));
                Encryptor no_pk(a.ctx, a.sk);
                check("encrypt_many without a public key throws" + how,
                      throws<std::logic_error>("public key is not set",
                                               [&] { no_pk.encrypt_many(first(p0, 3), mptrs(dest)); }));
                check("encrypt_zero_many without a public key throws" + how,
                      throws<std::logic_error>("public key is not set", [&] { no_pk.encrypt_zero_many(id0, mptrs(dest)); }));
                check("and every destination keeps its words" + how, all_same(dest, keep));
                std::vector<Plaintext> mixed = { p0[0], p1[1], p0[2] };
                bool threw = false;
                try
                {
                    a.enc->encrypt_many(first(mixed, 3), mptrs(dest));
                }
                catch (const std::invalid_argument &)
                {
                    threw = true;
                }
                check("plaintexts at two levels throw std::invalid_argument" + how, threw);
                std::vector<Ciphertext *> twice = { &dest[0], &dest[1], &dest[0] };
                threw = false;
                try
                {
                    a.enc->encrypt_many(first(p0, 3), twice);
                }
                catch (const std::invalid_argument &)
                {
                    threw = true;
                }
                check("a destination given twice throws std::invalid_argument" + how, threw);
                check("and every destination keeps its words" + how, all_same(dest, keep));
            }
            set_batched_launches(true);
        }
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
