// CKKSEncoder::encode_many (not SEAL API) against one encode call per vector, word for word, at
// N = 2^13 and three limbs: 11 real and 11 complex vectors (a full round of 8 and a remainder), the
// same with batched launches off, inside three FiberBatch fibers, a batch with one oversized vector
// (throws and every destination keeps its words, with batched launches on and off) and vectors of
// unequal sizes (throws).
//   encode_many_test
#include "seal/seal.h"

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

using namespace seal;

static int g_fail = 0;
static void check(const std::string &what, bool ok)
{
    std::printf("[%s] %s\n", ok ? "PASS" : "FAIL", what.c_str());
    if (!ok) g_fail++;
}
static bool same(const Plaintext &a, const Plaintext &b)
{
    if (a.scale() != b.scale() || a.parms_id() != b.parms_id() || a.limbs() != b.limbs()) return false;
    const PolyStore &x = a.store(), &y = b.store();
    return x.words() == y.words() && std::memcmp(x.host(), y.host(), x.words() * 8) == 0;
}
template <class T>
static std::vector<const T *> ptrs(const std::vector<T> &v)
{
    std::vector<const T *> p;
    for (const T &x : v) p.push_back(&x);
    return p;
}
static std::vector<Plaintext *> mptrs(std::vector<Plaintext> &v)
{
    std::vector<Plaintext *> p;
    for (Plaintext &x : v) p.push_back(&x);
    return p;
}
static bool all_same(const std::vector<Plaintext> &a, const std::vector<Plaintext> &b)
{
    bool ok = a.size() == b.size();
    for (std::size_t i = 0; ok && i < a.size(); i++) ok = same(a[i], b[i]);
    return ok;
}

int main()
{
    const std::size_t N = (std::size_t)1 << 13, slots = N / 2, M = 11;
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(N);
    parms.set_coeff_modulus(CoeffModulus::Create(N, { 51, 46, 46, 51 }));
    SEALContext ctx(parms, true, sec_level_type::none);
    CKKSEncoder encoder(ctx);
    const parms_id_type id = ctx.first_parms_id();
    const double scale = std::pow(2.0, 40);
    std::mt19937_64 g(5);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    try
    {
        std::vector<std::vector<double>> re(M, std::vector<double>(slots));
        std::vector<std::vector<std::complex<double>>> cx(M, std::vector<std::complex<double>>(slots));
        for (std::size_t i = 0; i < M; i++)
            for (std::size_t k = 0; k < slots; k++)
            {
                re[i][k] = U(g);
                cx[i][k] = { U(g), U(g) };
            }
        std::vector<Plaintext> want_re(M), want_cx(M);
        for (std::size_t i = 0; i < M; i++)
        {
            encoder.encode(re[i], id, scale, want_re[i]);
            encoder.encode(cx[i], id, scale, want_cx[i]);
        }
        check("the level has three limbs", want_re[0].limbs() == 3);
        for (int batched = 1; batched >= 0; batched--)
        {
            set_batched_launches(batched != 0);
            std::vector<Plaintext> got_re(M), got_cx(M);
            encoder.encode_many(ptrs(re), id, scale, mptrs(got_re));
            encoder.encode_many(ptrs(cx), id, scale, mptrs(got_cx));
            const std::string how = batched ? " (batched launches)" : " (batched launches off)";
            check("encode_many of 11 real vectors == 11 encode calls" + how, all_same(got_re, want_re));
            check("encode_many of 11 complex vectors == 11 encode calls" + how, all_same(got_cx, want_cx));
        }
        set_batched_launches(true);
        {
            // three fibers, each with its own batch: the same words (encodes are not merged across fibers)
            const std::size_t F = 3, per = 3;
            std::vector<std::vector<Plaintext>> got(F, std::vector<Plaintext>(per));
            FiberBatch::run(F, [&](std::size_t f) {
                std::vector<const std::vector<double> *> in;
                for (std::size_t k = 0; k < per; k++) in.push_back(&re[f * per + k]);
                encoder.encode_many(in, id, scale, mptrs(got[f]));
            });
            bool ok = true;
            for (std::size_t f = 0; f < F; f++)
                for (std::size_t k = 0; k < per; k++) ok = ok && same(got[f][k], want_re[f * per + k]);
            check("FiberBatch (3 fibers): each fiber's encode_many == encode", ok);
        }
        {
            // one oversized vector in the batch: 2^(tb-2) / scale * (1 + 2^-20) in every slot
            const int tb = ctx.first_context_data()->total_coeff_modulus_bit_count();
            std::vector<std::vector<double>> v(re.begin(), re.begin() + 3);
            v[1].assign(slots, std::ldexp(1.0, tb - 2) / scale * (1.0 + std::ldexp(1.0, -20)));
            for (int batched = 1; batched >= 0; batched--)
            {
                set_batched_launches(batched != 0);
                const std::string how = batched ? " (batched launches)" : " (batched launches off)";
                std::vector<Plaintext> dest(want_cx.begin(), want_cx.begin() + 3);
                bool threw = false;
                try
                {
                    encoder.encode_many(ptrs(v), id, scale, mptrs(dest));
                }
                catch (const std::invalid_argument &e)
                {
                    threw = std::string(e.what()) == "encoded values are too large";
                    std::printf("  %s\n", e.what());
                }
                check("an oversized vector in the batch throws \"encoded values are too large\"" + how, threw);
                check("and every destination keeps its words" + how,
                      all_same(dest, std::vector<Plaintext>(want_cx.begin(), want_cx.begin() + 3)));
            }
            set_batched_launches(true);
            // the same vector alone is rejected by encode as well
            bool single = false;
            try
            {
                Plaintext p;
                encoder.encode(v[1], id, scale, p);
            }
            catch (const std::invalid_argument &)
            {
                single = true;
            }
            check("encode rejects that vector too", single);
        }
        {
            std::vector<std::vector<double>> v(re.begin(), re.begin() + 3);
            v[2].resize(slots - 1);
            std::vector<Plaintext> dest(3);
            bool threw = false;
            try
            {
                encoder.encode_many(ptrs(v), id, scale, mptrs(dest));
            }
            catch (const std::invalid_argument &)
            {
                threw = true;
            }
            check("vectors of unequal sizes throw std::invalid_argument", threw);
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
