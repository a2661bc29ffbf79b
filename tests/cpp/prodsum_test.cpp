// Evaluator::multiply_sum_rescale (not SEAL API) against the sequence it is defined as --
// multiply_reduced_error per product, add_inplace_reduced_error over each sum in order, the sum added
// to itself when doubled, rescale_to_next_inplace -- word for word, scale for scale and parms_id for
// parms_id, on seeded keys at N = 2^13: sums of one to nine products, doubled or not; operands at
// unequal levels (the pre-adjustment of multiply_reduced_error); sums at two levels in one call; a sum
// whose products end at different levels, batched launches off and a level of one limb (the sequence
// itself runs); the calls of three FiberBatch fibers merged into one mhe_relin_sum_rescale; an
// injected scratch allocation failure that must leave the destinations' words alone.
//   prodsum_test
// and one composite ReLU (comp_test's setting) with seal::set_merged_product_sums off and on: equal
// words and scale, mhe_prodsum_stats nonzero only in the second run.
//   prodsum_test relu
#include "mhe_cnn.h"
#include "seal/seal.h"
#include "../../include/mhe.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

using namespace seal;

static int g_fail = 0;
static bool same(const Ciphertext &a, const Ciphertext &b)
{
    if (a.size() != b.size() || a.coeff_modulus_size() != b.coeff_modulus_size() || a.scale() != b.scale() ||
        a.parms_id() != b.parms_id() || a.is_ntt_form() != b.is_ntt_form())
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
static Stats prodsum_stats(const SEALContext &ctx, bool reset = false)
{
    Stats s;
    mhe_prodsum_stats(ctx.engine(), &s.sums, &s.terms, reset ? 1 : 0);
    return s;
}
static std::shared_ptr<UniformRandomGeneratorFactory> seeded(std::uint64_t a)
{
    return std::make_shared<Blake2xbPRNGFactory>(std::array<std::uint64_t, 8>{ a, 7, 1, 8, 2, 8, 1, 8 });
}
static std::vector<const Ciphertext *> ptrs(const std::vector<Ciphertext> &v)
{
    std::vector<const Ciphertext *> p;
    for (const Ciphertext &c : v) p.push_back(&c);
    return p;
}
static std::vector<Ciphertext *> mptrs(std::vector<Ciphertext> &v)
{
    std::vector<Ciphertext *> p;
    for (Ciphertext &c : v) p.push_back(&c);
    return p;
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
    parms.set_random_generator(seeded(3));
    SEALContext ctx(parms, true, sec_level_type::none);
    KeyGenerator keygen(ctx);
    PublicKey pk;
    keygen.create_public_key(pk);
    RelinKeys rlk;
    keygen.create_relin_keys(rlk);
    CKKSEncoder encoder(ctx);
    Encryptor encryptor(ctx, pk);
    Evaluator ev(ctx, encoder);
    const int slots = (int)N / 2;
    std::mt19937_64 g(14);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
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
    // the definition, call by call
    auto sequence = [&](const std::vector<const Ciphertext *> &a, const std::vector<const Ciphertext *> &b,
                        const std::vector<int> &group, const std::vector<bool> &twice, std::vector<Ciphertext> &out) {
        std::vector<Ciphertext> p(a.size());
        for (std::size_t i = 0; i < a.size(); i++) ev.multiply_reduced_error(*a[i], *b[i], rlk, p[i]);
        out.assign(twice.size(), Ciphertext());
        for (std::size_t gi = 0; gi < twice.size(); gi++)
        {
            Ciphertext d;
            bool started = false;
            for (std::size_t i = 0; i < a.size(); i++)
            {
                if (group[i] != (int)gi) continue;
                if (!started)
                    d = p[i];
                else
                    ev.add_inplace_reduced_error(d, p[i]);
                started = true;
            }
            if (twice[gi]) ev.add_inplace_reduced_error(d, d);
            ev.rescale_to_next_inplace(d);
            out[gi] = d;
        }
    };
    try
    {
        struct Case
        {
            const char *name;
            std::vector<int> sizes;                    // terms per sum
            std::vector<bool> twice;
            std::vector<std::pair<int, int>> drops;    // per term: levels dropped of each factor
            std::size_t merged_sums, merged_terms;     // what mhe_prodsum_stats must report
        };
        auto flat = [](int terms, int da, int db) { return std::vector<std::pair<int, int>>((std::size_t)terms, { da, db }); };
        std::vector<Case> cases{
            { "one product", { 1 }, { false }, flat(1, 0, 0), 1, 1 },
            { "one product, doubled", { 1 }, { true }, flat(1, 2, 2), 1, 1 },
            { "spines of 3 and 1 and a doubled step", { 3, 1, 1 }, { false, false, true }, flat(5, 1, 1), 3, 5 },
            { "nine products in one sum (two key-switch launches)", { 9 }, { true }, flat(9, 3, 3), 1, 9 },
            { "factors at unequal levels (pre-adjusted)", { 2, 1 }, { false, true }, flat(3, 0, 2), 2, 3 },
            { "sums at two levels in one call", { 2, 2 }, { true, false }, { { 1, 1 }, { 1, 1 }, { 3, 3 }, { 3, 3 } }, 2, 4 },
            { "a sum whose products end at different levels: the sequence", { 2 }, { false }, { { 1, 1 }, { 2, 2 } }, 0, 0 },
        };
        for (const Case &c : cases)
        {
            std::vector<Ciphertext> a, b;
            std::vector<int> group;
            for (std::size_t s = 0; s < c.sizes.size(); s++) group.insert(group.end(), (std::size_t)c.sizes[s], (int)s);
            for (std::size_t i = 0; i < group.size(); i++)
            {
                // every product at its own scale: a sum must come out at its last term's
                a.push_back(fresh(c.drops[i].first, std::pow(2.0, 46) * (1.0 + 0.0625 * i)));
                b.push_back(fresh(c.drops[i].second, std::pow(2.0, 46) * (1.0 + 0.0625 * i)));
            }
            const std::vector<Ciphertext> ka = a, kb = b;
            std::vector<Ciphertext> want, got(c.sizes.size());
            sequence(ptrs(a), ptrs(b), group, c.twice, want);
            prodsum_stats(ctx, true);
            ev.multiply_sum_rescale(ptrs(a), ptrs(b), group, c.twice, rlk, mptrs(got));
            const Stats st = prodsum_stats(ctx, true);
            bool ok = st.sums == c.merged_sums && st.terms == c.merged_terms;
            for (std::size_t s = 0; s < got.size(); s++) ok = ok && same(got[s], want[s]) && got[s].size() == 2;
            for (std::size_t i = 0; i < a.size(); i++) ok = ok && same(a[i], ka[i]) && same(b[i], kb[i]);
            check(std::string("multiply_sum_rescale == the sequence: ") + c.name, ok);
        }
        {
            // squares: both factors the same object
            std::vector<Ciphertext> a{ fresh(1, std::pow(2.0, 46)), fresh(1, std::pow(2.0, 46)) };
            std::vector<Ciphertext> want, got(1);
            sequence(ptrs(a), ptrs(a), { 0, 0 }, { true }, want);
            ev.multiply_sum_rescale(ptrs(a), ptrs(a), { 0, 0 }, { true }, rlk, mptrs(got));
            check("multiply_sum_rescale of squares == the sequence", same(got[0], want[0]));
        }
        {
            // batched launches off: the sequence, nothing merged
            std::vector<Ciphertext> a{ fresh(1, std::pow(2.0, 46)), fresh(1, std::pow(2.0, 46)) }, b = a;
            std::vector<Ciphertext> want, got(1);
            sequence(ptrs(a), ptrs(b), { 0, 0 }, { false }, want);
            prodsum_stats(ctx, true);
            set_batched_launches(false);
            ev.multiply_sum_rescale(ptrs(a), ptrs(b), { 0, 0 }, { false }, rlk, mptrs(got));
            set_batched_launches(true);
            const Stats st = prodsum_stats(ctx, true);
            check("batched launches off: the sequence's words, nothing merged", same(got[0], want[0]) && st.sums == 0);
        }
        {
            // the sequence's exceptions: the last level cannot be rescaled; bad arguments
            std::vector<Ciphertext> a{ fresh(6, std::pow(2.0, 20)) }, got(1);
            got[0] = fresh(2, std::pow(2.0, 40));
            const Ciphertext before = got[0];
            std::string seq_what, got_what;
            try
            {
                std::vector<Ciphertext> want;
                sequence(ptrs(a), ptrs(a), { 0 }, { false }, want);
            }
            catch (const std::exception &e)
            {
                seq_what = e.what();
            }
            try
            {
                ev.multiply_sum_rescale(ptrs(a), ptrs(a), { 0 }, { false }, rlk, mptrs(got));
            }
            catch (const std::exception &e)
            {
                got_what = e.what();
            }
            std::printf("  one limb: \"%s\"\n", got_what.c_str());
            check("a level of one limb throws what the sequence throws, destination unchanged",
                  !got_what.empty() && got_what == seq_what && same(got[0], before));
            auto throws = [&](const std::vector<int> &group, const std::vector<bool> &twice, std::vector<Ciphertext *> dst) {
                std::vector<Ciphertext> x{ fresh(1, std::pow(2.0, 46)), fresh(1, std::pow(2.0, 46)) };
                if (dst.empty()) dst = { &x[0] }; // a destination that is an input
                try
                {
                    ev.multiply_sum_rescale(ptrs(x), ptrs(x), group, twice, rlk, dst);
                }
                catch (const std::invalid_argument &)
                {
                    return true;
                }
                return false;
            };
            Ciphertext d0, d1;
            check("bad arguments throw std::invalid_argument",
                  throws({ 0, 0 }, { false }, {}) && throws({ 1, 1 }, { false, false }, { &d0, &d1 }) &&
                      throws({ 0, 2 }, { false, false }, { &d0, &d1 }) && throws({ 0, 1 }, { false }, { &d0, &d1 }) &&
                      throws({ 0, 1 }, { false, false }, { &d0, &d0 }) && throws({ 0 }, { false }, { &d0 }));
        }
        {
            // three fibers, the same-numbered call of each merged into one engine call
            const std::size_t M = 3;
            const std::vector<int> group{ 0, 0, 1 };
            const std::vector<bool> twice{ false, true };
            std::vector<std::vector<Ciphertext>> a(M), b(M), alone(M), fibered(M);
            for (std::size_t m = 0; m < M; m++)
                for (std::size_t i = 0; i < group.size(); i++)
                {
                    a[m].push_back(fresh(1, std::pow(2.0, 46)));
                    b[m].push_back(fresh(1, std::pow(2.0, 46)));
                }
            for (std::size_t m = 0; m < M; m++)
            {
                alone[m].resize(2);
                fibered[m].resize(2);
                ev.multiply_sum_rescale(ptrs(a[m]), ptrs(b[m]), group, twice, rlk, mptrs(alone[m]));
            }
            prodsum_stats(ctx, true);
            const std::uint64_t fb0 = merged_call_fallbacks();
            FiberBatch::run(M, [&](std::size_t m) {
                ev.multiply_sum_rescale(ptrs(a[m]), ptrs(b[m]), group, twice, rlk, mptrs(fibered[m]));
            });
            const Stats st = prodsum_stats(ctx, true);
            bool ok = true;
            for (std::size_t m = 0; m < M; m++) ok = ok && same(fibered[m][0], alone[m][0]) && same(fibered[m][1], alone[m][1]);
            std::printf("fibers: %zu member calls merged, %llu sums of %llu products\n", FiberBatch::last_merged(),
                        (unsigned long long)st.sums, (unsigned long long)st.terms);
            check("FiberBatch (3 fibers): each fiber's call == the same fiber alone", ok);
            check("FiberBatch: the three calls ran as one merged call",
                  FiberBatch::last_merged() >= M && st.sums == 2 * M && st.terms == 3 * M);
            check("FiberBatch: no merged call fell back", merged_call_fallbacks() == fb0);
        }
        {
            // the first merged call at the top level (every one above ran lower): its accumulators have
            // to grow.  With that growth failing, the call throws and the destinations keep their words
            std::vector<Ciphertext> a, b;
            for (int i = 0; i < 3; i++)
            {
                a.push_back(fresh(0, std::pow(2.0, 46)));
                b.push_back(fresh(0, std::pow(2.0, 46)));
            }
            const std::vector<int> group{ 0, 0, 1 };
            const std::vector<bool> twice{ false, true };
            std::vector<Ciphertext> want;
            sequence(ptrs(a), ptrs(b), group, twice, want);
            // the allocations of one call, counted: the products' stores, the results' stores, then
            // the engine's accumulators; every one of them failing in turn
            bool ok = true;
            int threw_count = 0;
            for (int nth = 1; nth <= 12; nth++)
            {
                std::vector<Ciphertext> dest{ fresh(2, std::pow(2.0, 40)), fresh(2, std::pow(2.0, 40)) };
                const std::vector<Ciphertext> before = dest;
                mhe_debug_fail_alloc(ctx.engine(), nth);
                bool threw = false;
                try
                {
                    ev.multiply_sum_rescale(ptrs(a), ptrs(b), group, twice, rlk, mptrs(dest));
                }
                catch (const std::exception &e)
                {
                    threw = true;
                    threw_count++;
                }
                mhe_debug_fail_alloc(ctx.engine(), 0);
                if (threw)
                    ok = ok && same(dest[0], before[0]) && same(dest[1], before[1]);
                else
                    ok = ok && same(dest[0], want[0]) && same(dest[1], want[1]);
            }
            std::printf("  %d of 12 injected allocation failures hit the call\n", threw_count);
            check("a failing allocation throws and leaves the destinations' words (or never hit the call)",
                  ok && threw_count > 0);
            std::vector<Ciphertext> dest(2);
            ev.multiply_sum_rescale(ptrs(a), ptrs(b), group, twice, rlk, mptrs(dest));
            check("multiply_sum_rescale after the failed calls == the sequence", same(dest[0], want[0]) && same(dest[1], want[1]));
        }
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\n", e.what());
        g_fail++;
    }
    return g_fail;
}

// one composite ReLU (comp_test's setting), merged product sums off and on
static int run_relu()
{
    const long comp_no = 3, alpha = 13;
    std::vector<int> deg = { 15, 15, 27 };
    std::vector<Tree> tree;
    for (int d : deg)
    {
        Tree tr;
        upgrade_oddbaby(d, tr);
        tree.push_back(tr);
    }
    EncryptionParameters parms(scheme_type::ckks);
    const std::size_t N = 1 << 13;
    parms.set_poly_modulus_degree(N);
    std::vector<int> bits(1, 51);
    for (int i = 0; i < 20; i++) bits.push_back(46);
    bits.push_back(51);
    parms.set_coeff_modulus(CoeffModulus::Create(N, bits));
    parms.set_random_generator(seeded(5)); // the encryptions inside the ReLU repeat from run to run
    SEALContext ctx(parms, true, sec_level_type::none);
    KeyGenerator keygen(ctx);
    PublicKey pk;
    keygen.create_public_key(pk);
    RelinKeys rlk;
    keygen.create_relin_keys(rlk);
    SecretKey sk = keygen.secret_key();
    CKKSEncoder encoder(ctx);
    Encryptor encryptor(ctx, pk);
    Decryptor decryptor(ctx, sk);
    Evaluator evaluator(ctx, encoder);
    const std::size_t slots = N / 2;
    std::mt19937_64 rng(3);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<double> x(slots);
    for (auto &v : x) v = u(rng);
    Plaintext pt;
    encoder.encode(x, std::pow(2.0, 46), pt);
    Ciphertext ct;
    encryptor.encrypt(pt, ct);
    try
    {
        Ciphertext out[2];
        Stats st[2];
        const bool was = merged_product_sums();
        for (int on = 0; on < 2; on++)
        {
            Ciphertext in = ct;
            set_merged_product_sums(on != 0);
            prodsum_stats(ctx, true);
            minimax_ReLU_seal(comp_no, deg, alpha, tree, 1.7, 46, encryptor, evaluator, decryptor, encoder, pk, sk, rlk, in,
                              out[on]);
            st[on] = prodsum_stats(ctx, true);
            std::printf("merged product sums %s: %llu sums of %llu products\n", on ? "on" : "off",
                        (unsigned long long)st[on].sums, (unsigned long long)st[on].terms);
        }
        set_merged_product_sums(was);
        decryptor.decrypt(out[1], pt);
        std::vector<double> y;
        encoder.decode(pt, y);
        double err = 0;
        for (std::size_t i = 0; i < slots; i++) err = std::max(err, std::fabs(y[i] - (x[i] > 0 ? x[i] : 0.0)));
        std::printf("ReLU: max abs error %.3g\n", err);
        check("ReLU with merged product sums: the words and scale of the ReLU without", same(out[0], out[1]));
        check("the ReLU decrypts to max(x, 0)", err < 5e-3);
        check("mhe_prodsum_stats: zero with the switch off, nonzero with it on",
              st[0].sums == 0 && st[0].terms == 0 && st[1].sums > 0 && st[1].terms >= st[1].sums);
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
    const int fails = (argc > 1 && std::string(argv[1]) == "relu") ? run_relu() : run_sums();
    std::printf(fails ? "%d FAILED\n" : "ALL PASSED\n", fails);
    return fails ? 1 : 0;
}
