// Pins the observable behaviour of seal::Evaluator (libmhe_seal.so) at N = 2^12 on the small chain of
// seal_api_test.cpp, so that a refactor of the evaluator's host code can be checked against it:
//   a. exception table: for every entry point and precondition the exception's exact type and text,
//      and every operand unchanged (words, size, parms_id, scale, NTT flag) after the throw;
//   b. alias matrix: every out-of-place entry point with a fresh destination, a destination holding
//      a larger ciphertext of another level, destination == first input and destination == second
//      input, word for word against the in-place form on a copy;
//   c. launch fingerprint: one fixed script over every entry point and the batched mixes, run
//      directly, in a FiberBatch of 3 fibers and in a Lockstep group of 3 threads: the engine's
//      per-kind, per-level operation counts and the merge counters, as literals.
// Cases seal_api_test.cpp / seal_batch_test.cpp cover are not repeated.  Driven by
// tests/test_seal_api.py (GPU marker).
#include "seal/seal.h"
#include "../../include/mhe.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>
#include <typeinfo>
#include <vector>

using namespace seal;
using IA = std::invalid_argument;
using LE = std::logic_error;
using CtIn = std::vector<const Ciphertext *>;
using CtOut = std::vector<Ciphertext *>;

static int g_fail = 0, g_checks = 0;
static void check(const std::string &what, bool ok)
{
    g_checks++;
    if (!ok)
    {
        g_fail++;
        std::printf("[FAIL] %s\n", what.c_str());
    }
}

struct Snap
{
    std::vector<std::uint64_t> w;
    std::size_t size = 0;
    parms_id_type id{};
    double scale = 0;
    bool ntt = false;
    bool operator==(const Snap &o) const
    {
        return w == o.w && size == o.size && id == o.id && std::memcmp(&scale, &o.scale, 8) == 0 && ntt == o.ntt;
    }
};
static Snap snap(const Ciphertext &c)
{
    Snap s;
    s.size = c.size();
    s.id = c.parms_id();
    s.scale = c.scale();
    s.ntt = c.is_ntt_form();
    const std::size_t n = c.store().words();
    if (n && c.store().engine())
    {
        const std::uint64_t *h = c.store().host();
        s.w.assign(h, h + n);
    }
    return s;
}
static bool same(const Ciphertext &a, const Ciphertext &b)
{
    return snap(a) == snap(b);
}
static CtIn cp(std::initializer_list<const Ciphertext *> l)
{
    return CtIn(l);
}

// f() must throw exactly E with text msg and leave every ciphertext of ops as it was
template <class E, class F>
static void throws_exact(const char *call, const std::string &msg, const CtIn &ops, F f)
{
    std::vector<Snap> before;
    for (const Ciphertext *c : ops) before.push_back(snap(*c));
    std::string got = "(no exception)";
    bool type_ok = false;
    try
    {
        f();
    }
    catch (const std::exception &e)
    {
        got = e.what();
        type_ok = typeid(e) == typeid(E);
    }
    bool kept = true;
    for (std::size_t i = 0; i < ops.size(); i++) kept = kept && before[i] == snap(*ops[i]);
    check(std::string(call) + " -> \"" + msg + "\"; got \"" + got + "\"" + (type_ok ? "" : " (other type)") +
              (kept ? "" : " (operand changed)"),
          type_ok && got == msg && kept);
}
#define X(E, MSG, OPS, ...) throws_exact<E>(#__VA_ARGS__, MSG, OPS, [&] { __VA_ARGS__; })

int main()
{
    const std::size_t N = 4096;
    const int logN = 12, slots = (int)N / 2;
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(N);
    parms.set_coeff_modulus(CoeffModulus::Create(N, { 60, 40, 40, 40, 40, 60 }));
    parms.set_random_generator(
        std::make_shared<Blake2xbPRNGFactory>(std::array<std::uint64_t, 8>{ 2, 7, 1, 8, 2, 8, 1, 8 }));
    SEALContext ctx(parms, true, sec_level_type::none);
    KeyGenerator keygen(ctx);
    PublicKey pk;
    keygen.create_public_key(pk);
    RelinKeys rlk;
    keygen.create_relin_keys(rlk);
    // keys for steps 1, 2, 4, -1: step 3 = 4 - 1 runs SEAL's NAF path, steps 8 and 24 have no key
    GaloisKeys glk, gconj;
    keygen.create_galois_keys(std::vector<int>{ 1, 2, 4, -1 }, glk);
    keygen.create_galois_keys_from_elts({ (std::uint32_t)(2 * N - 1) }, gconj);
    CKKSEncoder encoder(ctx);
    Encryptor encryptor(ctx, pk);
    Evaluator ev(ctx, encoder);
    const double S = std::pow(2.0, 30);
    const parms_id_type first = ctx.first_parms_id(), last = ctx.last_parms_id();
    const parms_id_type low = ctx.first_context_data()->next_context_data()->parms_id();
    const parms_id_type zero = parms_id_zero, junk = { 1, 2, 3, 4 };
    const std::uint32_t e1 = mhe_galois_elt_from_step(logN, 1), e8 = mhe_galois_elt_from_step(logN, 8);
    int seed = 0;
    auto values = [&] {
        std::vector<double> v(slots);
        for (int i = 0; i < slots; i++) v[i] = std::sin(0.37 * i + (double)seed);
        seed++;
        return v;
    };
    auto plain = [&](parms_id_type id, double scale) {
        Plaintext p;
        encoder.encode(values(), id, scale, p);
        return p;
    };
    auto fresh = [&](parms_id_type id) {
        Ciphertext c;
        encryptor.encrypt(plain(first, S), c);
        if (id != first) ev.mod_switch_to_inplace(c, id);
        return c;
    };
    // "scale out of bounds" as check_scale prints it
    auto oob = [&](double scale, parms_id_type id) {
        auto cd = ctx.get_context_data(id);
        return "scale out of bounds (2^" + std::to_string(std::log2(scale)) + " at " +
               std::to_string(cd->parms().coeff_modulus().size()) + " limbs, " +
               std::to_string((double)cd->total_coeff_modulus_bit_count()) + " bits)";
    };
    const std::string NV = " is not valid for encryption parameters";
    try
    {
        // ------------------------------------------------------------------ a. exception table
        Ciphertext A = fresh(first), B = fresh(first), LOW = fresh(low), LOW2 = fresh(low), LAST = fresh(last), EMPTY, C3,
                   C3b;
        ev.multiply(A, B, C3);
        C3b = C3;
        Ciphertext COEFF = A, COEFF2 = B, C3COEFF = C3, HUGE = A, HUGE2 = A, C3S = C3;
        C3S.scale() = S; // (the in-place reduced-error forms copy encrypted2's scale before their checks)
        COEFF.is_ntt_form() = COEFF2.is_ntt_form() = C3COEFF.is_ntt_form() = false;
        HUGE.scale() = std::pow(2.0, 150);
        HUGE2.scale() = std::pow(2.0, 250);
        Plaintext P = plain(first, S), PLOW = plain(low, S), PLAST = plain(last, S), PNONE, PBAD = P;
        PBAD.parms_id() = junk;
        RelinKeys rbad, rnokey;
        rnokey.parms_id() = ctx.key_parms_id();
        GaloisKeys gbad;
        Ciphertext D, D2;
        const double q_last = (double)ctx.first_context_data()->parms().coeff_modulus().back().value();

        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.negate_inplace(EMPTY));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.negate(EMPTY, D));
        {
            struct Bin
            {
                const char *name;
                std::function<void(Ciphertext &, const Ciphertext &)> ip;
                std::function<void(const Ciphertext &, const Ciphertext &, Ciphertext &)> op;
            };
            const Bin bins[] = {
                { "add", [&](Ciphertext &a, const Ciphertext &b) { ev.add_inplace(a, b); },
                  [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.add(a, b, d); } },
                { "sub", [&](Ciphertext &a, const Ciphertext &b) { ev.sub_inplace(a, b); },
                  [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.sub(a, b, d); } },
            };
            for (const Bin &b : bins)
            {
                const std::string n = b.name;
                throws_exact<IA>((n + "_inplace(EMPTY, B)").c_str(), "encrypted1" + NV, cp({ &EMPTY, &B }), [&] { b.ip(EMPTY, B); });
                throws_exact<IA>((n + "_inplace(A, EMPTY)").c_str(), "encrypted2" + NV, cp({ &A, &EMPTY }), [&] { b.ip(A, EMPTY); });
                throws_exact<IA>((n + "_inplace(A, LOW)").c_str(), "encrypted1 and encrypted2 parameter mismatch", cp({ &A, &LOW }), [&] { b.ip(A, LOW); });
                throws_exact<IA>((n + "_inplace(A, COEFF)").c_str(), "NTT form mismatch", cp({ &A, &COEFF }), [&] { b.ip(A, COEFF); });
                throws_exact<IA>((n + "_inplace(A, HUGE)").c_str(), "scale mismatch", cp({ &A, &HUGE }), [&] { b.ip(A, HUGE); });
                throws_exact<IA>((n + "(EMPTY, B, D)").c_str(), "encrypted1" + NV, cp({ &EMPTY, &B }), [&] { Ciphertext d; b.op(EMPTY, B, d); });
                throws_exact<IA>((n + "(A, EMPTY, D)").c_str(), "encrypted2" + NV, cp({ &A, &EMPTY }), [&] { Ciphertext d; b.op(A, EMPTY, d); });
                throws_exact<IA>((n + "(A, LOW, D)").c_str(), "encrypted1 and encrypted2 parameter mismatch", cp({ &A, &LOW }), [&] { Ciphertext d; b.op(A, LOW, d); });
                throws_exact<IA>((n + "(A, COEFF, D)").c_str(), "NTT form mismatch", cp({ &A, &COEFF }), [&] { Ciphertext d; b.op(A, COEFF, d); });
                throws_exact<IA>((n + "(A, HUGE, D)").c_str(), "scale mismatch", cp({ &A, &HUGE }), [&] { Ciphertext d; b.op(A, HUGE, d); });
            }
        }
        X(IA, "encrypteds cannot be empty", cp({ &D }), ev.add_many({}, D));
        {
            std::vector<Ciphertext> v{ A, B };
            X(IA, "encrypteds must be different from destination", cp({ &v[0], &v[1] }), ev.add_many(v, v[1]));
            X(IA, "encrypteds vector must not be empty", cp({ &D }), ev.multiply_many({}, rlk, D));
            X(IA, "encrypteds must be different from destination", cp({ &v[0], &v[1] }), ev.multiply_many(v, rlk, v[0]));
            X(LE, "unsupported scheme", cp({ &v[0], &v[1] }), ev.multiply_many(v, rlk, D));
            std::vector<Ciphertext> e{ EMPTY };
            X(IA, "encrypteds" + NV, cp({ &e[0] }), ev.multiply_many(e, rlk, D));
        }
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.exponentiate_inplace(EMPTY, 2, rlk));
        X(IA, "relin_keys" + NV, cp({ &A }), ev.exponentiate_inplace(A, 2, rbad));
        X(IA, "exponent cannot be 0", cp({ &A }), ev.exponentiate_inplace(A, 0, rlk));
        X(LE, "unsupported scheme", cp({ &A }), ev.exponentiate_inplace(A, 2, rlk));

        // ciphertext product
        X(IA, "encrypted1" + NV, cp({ &EMPTY, &B }), ev.multiply_inplace(EMPTY, B));
        X(IA, "encrypted2" + NV, cp({ &A, &EMPTY }), ev.multiply_inplace(A, EMPTY));
        X(IA, "encrypted1 and encrypted2 parameter mismatch", cp({ &A, &LOW }), ev.multiply_inplace(A, LOW));
        X(IA, "encrypted1 or encrypted2 must be in NTT form", cp({ &A, &COEFF }), ev.multiply_inplace(A, COEFF));
        X(IA, "encrypted1 or encrypted2 must be in NTT form", cp({ &COEFF, &B }), ev.multiply_inplace(COEFF, B));
        X(LE, "only size-2 ciphertexts are multiplied (relinearize first)", cp({ &C3, &B }), ev.multiply_inplace(C3, B));
        X(LE, "only size-2 ciphertexts are multiplied (relinearize first)", cp({ &A, &C3 }), ev.multiply_inplace(A, C3));
        X(IA, oob(std::pow(2.0, 300), first), cp({ &HUGE }), ev.multiply_inplace(HUGE, HUGE));
        X(IA, "encrypted1" + NV, cp({ &EMPTY, &B }), ev.multiply(EMPTY, B, D));
        X(IA, "encrypted2" + NV, cp({ &A, &EMPTY }), ev.multiply(A, EMPTY, D));
        X(IA, "encrypted1 and encrypted2 parameter mismatch", cp({ &A, &LOW }), ev.multiply(A, LOW, D));
        X(IA, "encrypted1 or encrypted2 must be in NTT form", cp({ &A, &COEFF }), ev.multiply(A, COEFF, D));
        X(LE, "only size-2 ciphertexts are multiplied (relinearize first)", cp({ &C3, &B }), ev.multiply(C3, B, D));
        X(LE, "only size-2 ciphertexts are multiplied (relinearize first)", cp({ &A, &C3 }), ev.multiply(A, C3, D));
        X(IA, oob(std::pow(2.0, 300), first), cp({ &HUGE, &HUGE2 }), ev.multiply(HUGE, HUGE, D));

        // square
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.square_inplace(EMPTY));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF }), ev.square_inplace(COEFF));
        X(LE, "only size-2 ciphertexts are squared (relinearize first)", cp({ &C3 }), ev.square_inplace(C3));
        X(IA, oob(std::pow(2.0, 300), first), cp({ &HUGE }), ev.square_inplace(HUGE));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.square(EMPTY, D));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF }), ev.square(COEFF, D));
        X(LE, "only size-2 ciphertexts are squared (relinearize first)", cp({ &C3 }), ev.square(C3, D));
        X(IA, oob(std::pow(2.0, 300), first), cp({ &HUGE }), ev.square(HUGE, D));

        // relinearize
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.relinearize_inplace(EMPTY, rlk));
        X(IA, "relin_keys" + NV, cp({ &C3 }), ev.relinearize_inplace(C3, rbad));
        X(IA, "encrypted must be in NTT form", cp({ &C3COEFF }), ev.relinearize_inplace(C3COEFF, rlk));
        X(IA, "key-switching key is truncated below the ciphertext level", cp({ &C3 }), ev.relinearize_inplace(C3, rnokey));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.relinearize(EMPTY, rlk, D));
        X(IA, "relin_keys" + NV, cp({ &C3 }), ev.relinearize(C3, rbad, D));
        X(IA, "encrypted must be in NTT form", cp({ &C3COEFF }), ev.relinearize(C3COEFF, rlk, D));
        X(IA, "key-switching key is truncated below the ciphertext level", cp({ &C3 }), ev.relinearize(C3, rnokey, D));

        // modulus switching
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.mod_switch_to_next_inplace(EMPTY));
        X(IA, "CKKS encrypted must be in NTT form", cp({ &COEFF }), ev.mod_switch_to_next_inplace(COEFF));
        X(IA, "end of modulus switching chain reached", cp({ &LAST }), ev.mod_switch_to_next_inplace(LAST));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.mod_switch_to_next(EMPTY, D));
        X(IA, "CKKS encrypted must be in NTT form", cp({ &COEFF }), ev.mod_switch_to_next(COEFF, D));
        X(IA, "end of modulus switching chain reached", cp({ &LAST }), ev.mod_switch_to_next(LAST, D));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.mod_switch_to_inplace(EMPTY, low));
        X(IA, "parms_id" + NV, cp({ &A }), ev.mod_switch_to_inplace(A, zero));
        X(IA, "cannot switch to higher level modulus", cp({ &LOW }), ev.mod_switch_to_inplace(LOW, first));
        X(IA, "CKKS encrypted must be in NTT form", cp({ &COEFF }), ev.mod_switch_to_inplace(COEFF, low));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.mod_switch_to(EMPTY, low, D));
        X(IA, "parms_id" + NV, cp({ &A }), ev.mod_switch_to(A, zero, D));
        X(IA, "cannot switch to higher level modulus", cp({ &LOW }), ev.mod_switch_to(LOW, first, D));
        X(IA, "CKKS encrypted must be in NTT form", cp({ &COEFF }), ev.mod_switch_to(COEFF, low, D));
        X(IA, "plain is not in NTT form", cp({}), ev.mod_switch_to_next_inplace(PNONE));
        X(IA, "plain" + NV, cp({}), ev.mod_switch_to_next_inplace(PBAD));
        X(IA, "end of modulus switching chain reached", cp({}), ev.mod_switch_to_next_inplace(PLAST));
        X(IA, "plain" + NV, cp({}), ev.mod_switch_to_inplace(PBAD, low));
        X(IA, "plain" + NV, cp({}), ev.mod_switch_to_inplace(PNONE, low));
        X(IA, "parms_id" + NV, cp({}), ev.mod_switch_to_inplace(P, zero));
        X(IA, "cannot switch to higher level modulus", cp({}), ev.mod_switch_to_inplace(PLOW, first));
        check("plaintexts keep their level and scale after the throws",
              P.parms_id() == first && PLOW.parms_id() == low && PLAST.parms_id() == last && PBAD.parms_id() == junk &&
                  P.scale() == S && PLOW.scale() == S && PLAST.scale() == S);

        // rescale
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.rescale_to_next(EMPTY, D));
        X(IA, "end of modulus switching chain reached", cp({ &LAST }), ev.rescale_to_next(LAST, D));
        X(IA, "CKKS encrypted must be in NTT form", cp({ &COEFF }), ev.rescale_to_next(COEFF, D));
        X(IA, oob(HUGE2.scale() / q_last, low), cp({ &HUGE2 }), ev.rescale_to_next(HUGE2, D));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.rescale_to_next_inplace(EMPTY));
        X(IA, "end of modulus switching chain reached", cp({ &LAST }), ev.rescale_to_next_inplace(LAST));
        X(IA, "CKKS encrypted must be in NTT form", cp({ &COEFF }), ev.rescale_to_next_inplace(COEFF));
        X(IA, oob(HUGE2.scale() / q_last, low), cp({ &HUGE2 }), ev.rescale_to_next_inplace(HUGE2));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.rescale_to_inplace(EMPTY, low));
        X(IA, "parms_id" + NV, cp({ &A }), ev.rescale_to_inplace(A, zero));
        X(IA, "cannot switch to higher level modulus", cp({ &LOW }), ev.rescale_to_inplace(LOW, first));
        X(IA, "CKKS encrypted must be in NTT form", cp({ &COEFF }), ev.rescale_to_inplace(COEFF, low));

        // plaintext operands
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.multiply_plain_inplace(EMPTY, P));
        X(IA, "plain" + NV, cp({ &A }), ev.multiply_plain_inplace(A, PBAD));
        X(IA, "NTT form mismatch", cp({ &A }), ev.multiply_plain_inplace(A, PNONE));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF }), ev.multiply_plain_inplace(COEFF, PNONE));
        X(IA, "encrypted_ntt and plain_ntt parameter mismatch", cp({ &A }), ev.multiply_plain_inplace(A, PLOW));
        X(IA, oob(std::pow(2.0, 280), first), cp({ &HUGE2 }), ev.multiply_plain_inplace(HUGE2, P));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.multiply_plain(EMPTY, P, D));
        X(IA, "plain" + NV, cp({ &A }), ev.multiply_plain(A, PBAD, D));
        X(IA, "NTT form mismatch", cp({ &A }), ev.multiply_plain(A, PNONE, D));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF }), ev.multiply_plain(COEFF, PNONE, D));
        X(IA, "encrypted_ntt and plain_ntt parameter mismatch", cp({ &A }), ev.multiply_plain(A, PLOW, D));
        X(IA, oob(std::pow(2.0, 280), first), cp({ &HUGE2 }), ev.multiply_plain(HUGE2, P, D));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.add_plain_inplace(EMPTY, P));
        X(IA, "NTT form mismatch", cp({ &A }), ev.add_plain_inplace(A, PNONE));
        X(IA, "encrypted and plain parameter mismatch", cp({ &A }), ev.add_plain_inplace(A, PLOW));
        X(IA, "scale mismatch", cp({ &HUGE }), ev.add_plain_inplace(HUGE, P));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.add_plain(EMPTY, P, D));
        X(IA, "NTT form mismatch", cp({ &A }), ev.add_plain(A, PNONE, D));
        X(IA, "encrypted and plain parameter mismatch", cp({ &A }), ev.add_plain(A, PLOW, D));
        X(IA, "scale mismatch", cp({ &HUGE }), ev.add_plain(HUGE, P, D));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.sub_plain_inplace(EMPTY, P));
        X(IA, "NTT form mismatch", cp({ &A }), ev.sub_plain_inplace(A, PNONE));
        X(IA, "encrypted and plain parameter mismatch", cp({ &A }), ev.sub_plain_inplace(A, PLOW));
        X(IA, "scale mismatch", cp({ &HUGE }), ev.sub_plain_inplace(HUGE, P));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.sub_plain(EMPTY, P, D));
        X(IA, "NTT form mismatch", cp({ &A }), ev.sub_plain(A, PNONE, D));
        X(IA, "encrypted and plain parameter mismatch", cp({ &A }), ev.sub_plain(A, PLOW, D));
        X(IA, "scale mismatch", cp({ &HUGE }), ev.sub_plain(HUGE, P, D));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.transform_to_ntt_inplace(EMPTY));
        X(IA, "encrypted is already in NTT form", cp({ &A }), ev.transform_to_ntt_inplace(A));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.transform_from_ntt_inplace(EMPTY));
        X(IA, "encrypted is not in NTT form", cp({ &COEFF }), ev.transform_from_ntt_inplace(COEFF));

        // Galois
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.apply_galois_inplace(EMPTY, e1, glk));
        X(IA, "galois_keys" + NV, cp({ &A }), ev.apply_galois_inplace(A, e1, gbad));
        X(IA, "Galois element is not valid", cp({ &A }), ev.apply_galois_inplace(A, 2, glk));
        X(IA, "Galois element is not valid", cp({ &A }), ev.apply_galois_inplace(A, (std::uint32_t)(2 * N + 1), glk));
        X(IA, "encrypted size must be 2", cp({ &C3 }), ev.apply_galois_inplace(C3, e1, glk));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF }), ev.apply_galois_inplace(COEFF, e1, glk));
        X(IA, "Galois key not present", cp({ &A }), ev.apply_galois_inplace(A, e8, glk));
        X(IA, "encrypted" + NV, cp({ &EMPTY, &D }), ev.apply_galois_to(EMPTY, e1, glk, D));
        X(IA, "galois_keys" + NV, cp({ &A, &D }), ev.apply_galois_to(A, e1, gbad, D));
        X(IA, "Galois element is not valid", cp({ &A, &D }), ev.apply_galois_to(A, 2, glk, D));
        X(IA, "Galois element is not valid", cp({ &A, &D }), ev.apply_galois_to(A, (std::uint32_t)(2 * N + 1), glk, D));
        X(IA, "encrypted size must be 2", cp({ &C3, &D }), ev.apply_galois_to(C3, e1, glk, D));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF, &D }), ev.apply_galois_to(COEFF, e1, glk, D));
        X(IA, "Galois key not present", cp({ &A, &D }), ev.apply_galois_to(A, e8, glk, D));
        X(IA, "result cannot point to the same value as operand", cp({ &A }), ev.apply_galois_to(A, e1, glk, A));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.rotate_vector_inplace(EMPTY, 1, glk));
        X(IA, "galois_keys" + NV, cp({ &A }), ev.rotate_vector_inplace(A, 1, gbad));
        X(IA, "step count too large", cp({ &A }), ev.rotate_vector_inplace(A, slots, glk));
        X(IA, "encrypted size must be 2", cp({ &C3 }), ev.rotate_vector_inplace(C3, 1, glk));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF }), ev.rotate_vector_inplace(COEFF, 1, glk));
        X(IA, "Galois key not present", cp({ &A }), ev.rotate_vector_inplace(A, 8, glk));
        X(IA, "Galois key not present", cp({ &A }), ev.rotate_vector_inplace(A, 24, glk));
        X(IA, "encrypted" + NV, cp({ &EMPTY, &D }), ev.rotate_vector(EMPTY, 1, glk, D));
        X(IA, "galois_keys" + NV, cp({ &A, &D }), ev.rotate_vector(A, 1, gbad, D));
        X(IA, "step count too large", cp({ &A, &D }), ev.rotate_vector(A, -slots, glk, D));
        X(IA, "encrypted size must be 2", cp({ &C3, &D }), ev.rotate_vector(C3, 1, glk, D));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF, &D }), ev.rotate_vector(COEFF, 1, glk, D));
        X(IA, "Galois key not present", cp({ &A }), ev.rotate_vector(A, 8, glk, D2));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.complex_conjugate_inplace(EMPTY, gconj));
        X(IA, "galois_keys" + NV, cp({ &A }), ev.complex_conjugate_inplace(A, gbad));
        X(IA, "Galois key not present", cp({ &A }), ev.complex_conjugate_inplace(A, glk));
        X(IA, "encrypted" + NV, cp({ &EMPTY, &D }), ev.complex_conjugate(EMPTY, gconj, D));
        X(IA, "galois_keys" + NV, cp({ &A, &D }), ev.complex_conjugate(A, gbad, D));
        X(IA, "Galois key not present", cp({ &A, &D }), ev.complex_conjugate(A, glk, D));

        // scalar residues
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.add_const_inplace(EMPTY, 1.0));
        X(IA, "NTT form mismatch", cp({ &COEFF }), ev.add_const_inplace(COEFF, 1.0));
        X(IA, "encrypted" + NV, cp({ &EMPTY, &D }), ev.add_const(EMPTY, 1.0, D));
        X(IA, "NTT form mismatch", cp({ &COEFF, &D }), ev.add_const(COEFF, 1.0, D));
        X(IA, "encrypted" + NV, cp({ &EMPTY }), ev.multiply_const_inplace(EMPTY, 1.0));
        X(IA, "NTT form mismatch", cp({ &COEFF }), ev.multiply_const_inplace(COEFF, 1.0));
        X(IA, oob(std::pow(2.0, 300), first), cp({ &HUGE }), ev.multiply_const_inplace(HUGE, 1.0));
        X(IA, "encrypted" + NV, cp({ &EMPTY, &D }), ev.multiply_const(EMPTY, 1.0, D));
        X(IA, "NTT form mismatch", cp({ &COEFF, &D }), ev.multiply_const(COEFF, 1.0, D));
        X(IA, oob(std::pow(2.0, 300), first), cp({ &HUGE, &D }), ev.multiply_const(HUGE, 1.0, D));

        // fused plaintext products
        X(IA, "encrypted" + NV, cp({ &A, &EMPTY }), ev.multiply_plain_add_reduced_error(A, EMPTY, P));
        X(IA, "encrypted1" + NV, cp({ &EMPTY, &A }), ev.multiply_plain_add_reduced_error(EMPTY, A, P));
        X(IA, "multiply_plain_add: acc and encrypted must share level and size", cp({ &LOW, &A }),
          ev.multiply_plain_add_reduced_error(LOW, A, P));
        X(IA, "multiply_plain_add: acc and encrypted must share level and size", cp({ &C3, &A }),
          ev.multiply_plain_add_reduced_error(C3, A, P));
        X(IA, "NTT form mismatch", cp({ &A, &B }), ev.multiply_plain_add_reduced_error(A, B, PNONE));
        X(IA, "encrypted_ntt and plain_ntt parameter mismatch", cp({ &LOW, &LOW2 }),
          ev.multiply_plain_add_reduced_error(LOW, LOW2, P));
        X(IA, oob(std::pow(2.0, 280), first), cp({ &A, &HUGE2 }), ev.multiply_plain_add_reduced_error(A, HUGE2, P));
        X(IA, "encrypted and plain must be non-empty and of the same size", cp({ &D }), ev.multiply_plain_sum({}, {}, D));
        X(IA, "encrypted and plain must be non-empty and of the same size", cp({ &A, &D }), ev.multiply_plain_sum({ &A }, { &P, &P }, D));
        X(IA, "multiply_plain_sum: null operand or destination among the inputs", cp({ &A, &D }), ev.multiply_plain_sum({ &A }, { nullptr }, D));
        X(IA, "multiply_plain_sum: null operand or destination among the inputs", cp({ &A }), ev.multiply_plain_sum({ &A }, { &P }, A));
        X(IA, "multiply_plain_add: acc and encrypted must share level and size", cp({ &A, &LOW, &D }),
          ev.multiply_plain_sum({ &A, &LOW }, { &P, &PLOW }, D));
        X(IA, "NTT form mismatch", cp({ &A, &D }), ev.multiply_plain_sum({ &A }, { &PNONE }, D));
        X(IA, "encrypted_ntt and plain_ntt parameter mismatch", cp({ &A, &D }), ev.multiply_plain_sum({ &A }, { &PLOW }, D));

        // reduced-error forms
        X(IA, "NTT form mismatch", cp({ &A, &COEFF }), ev.add_inplace_reduced_error(A, COEFF));
        X(IA, "NTT form mismatch", cp({ &A, &COEFF }), ev.sub_inplace_reduced_error(A, COEFF));
        X(IA, "NTT form mismatch", cp({ &A, &COEFF, &D }), ev.add_reduced_error(A, COEFF, D));
        X(IA, "NTT form mismatch", cp({ &A, &COEFF, &D }), ev.sub_reduced_error(A, COEFF, D));
        X(IA, "encrypted1 or encrypted2 must be in NTT form", cp({ &A, &COEFF }), ev.multiply_inplace_reduced_error(A, COEFF, rlk));
        X(LE, "only size-2 ciphertexts are multiplied (relinearize first)", cp({ &A, &C3S }), ev.multiply_inplace_reduced_error(A, C3S, rlk));
        X(IA, "NTT form mismatch", cp({ &A, &COEFF, &D }), ev.multiply_reduced_error(A, COEFF, rlk, D));
        X(LE, "only size-2 ciphertexts are multiplied (relinearize first)", cp({ &A, &C3 }), ev.multiply_reduced_error(A, C3, rlk, D2));
        X(IA, oob(std::pow(2.0, 300), first), cp({ &A, &HUGE, &D }), ev.multiply_reduced_error(A, HUGE, rlk, D));
        X(IA, "relin_keys" + NV, cp({ &A, &B }), ev.multiply_reduced_error(A, B, rbad, D2));

        // batched forms (a destination keeps its contents)
        Ciphertext E1, E2;
        X(IA, "encrypted, steps and destinations must have the same size", cp({ &A, &E1 }), ev.rotate_vectors({ &A }, { 1, 2 }, glk, { &E1 }));
        X(IA, "encrypted, steps and destinations must have the same size", cp({ &A, &E1, &E2 }), ev.rotate_vectors({ &A }, { 1 }, glk, { &E1, &E2 }));
        X(IA, "null ciphertext", cp({ &E1 }), ev.rotate_vectors({ nullptr }, { 1 }, glk, { &E1 }));
        X(IA, "null ciphertext", cp({ &A }), ev.rotate_vectors({ &A }, { 1 }, glk, { nullptr }));
        X(IA, "destinations must be distinct and must not be inputs", cp({ &A, &B, &E1 }), ev.rotate_vectors({ &A, &B }, { 1, 1 }, glk, { &E1, &E1 }));
        X(IA, "destinations must be distinct and must not be inputs", cp({ &A, &B, &E1 }), ev.rotate_vectors({ &A, &B }, { 1, 2 }, glk, { &E1, &A }));
        X(IA, "galois_keys" + NV, cp({ &A, &E1 }), ev.rotate_vectors({ &A }, { 1 }, gbad, { &E1 }));
        X(IA, "encrypted" + NV, cp({ &A, &EMPTY, &E1, &E2 }), ev.rotate_vectors({ &A, &EMPTY }, { 1, 2 }, glk, { &E1, &E2 }));
        X(IA, "step count too large", cp({ &A, &B, &E1, &E2 }), ev.rotate_vectors({ &A, &B }, { 1, slots }, glk, { &E1, &E2 }));
        X(IA, "encrypted size must be 2", cp({ &C3, &C3b, &E1, &E2 }), ev.rotate_vectors({ &C3, &C3b }, { 1, 2 }, glk, { &E1, &E2 }));
        X(IA, "encrypted must be in NTT form", cp({ &COEFF, &COEFF2, &E1, &E2 }), ev.rotate_vectors({ &COEFF, &COEFF2 }, { 1, 2 }, glk, { &E1, &E2 }));
        X(IA, "encrypted and steps must have the same, nonzero size", cp({ &E1 }), ev.rotate_sum({}, {}, glk, E1));
        X(IA, "encrypted and steps must have the same, nonzero size", cp({ &A, &E1 }), ev.rotate_sum({ &A }, { 1, 2 }, glk, E1));
        X(IA, "null ciphertext", cp({ &A, &E1 }), ev.rotate_sum({ &A, nullptr }, { 1, 2 }, glk, E1));
        X(IA, "galois_keys" + NV, cp({ &A, &B, &E1 }), ev.rotate_sum({ &A, &B }, { 1, 2 }, gbad, E1));
        X(IA, "step count too large", cp({ &A, &B, &E1 }), ev.rotate_sum({ &A, &B }, { 1, slots }, glk, E1));
        X(IA, "Galois key not present", cp({ &A, &B }), ev.rotate_sum({ &A, &B }, { 1, 8 }, glk, D2));
        X(IA, "relin_keys" + NV, cp({ &C3 }), ev.relinearize_inplace_many({ &C3 }, rbad));
        X(IA, "null ciphertext", cp({ &C3 }), ev.relinearize_inplace_many({ &C3, nullptr }, rlk));
        X(IA, "entries must be distinct", cp({ &C3 }), ev.relinearize_inplace_many({ &C3, &C3 }, rlk));
        X(IA, "encrypted" + NV, cp({ &C3, &EMPTY, &C3b }), ev.relinearize_inplace_many({ &C3, &EMPTY, &C3b }, rlk));
        X(IA, "encrypted must be in NTT form", cp({ &C3, &C3COEFF, &C3b }), ev.relinearize_inplace_many({ &C3, &C3COEFF, &C3b }, rlk));
        X(IA, "key-switching key is truncated below the ciphertext level", cp({ &C3, &C3b }), ev.relinearize_inplace_many({ &C3, &C3b }, rnokey));
        X(IA, "encrypted1, encrypted2 and destinations must have the same size", cp({ &A, &B, &E1 }), ev.multiply_reduced_error_many({ &A, &B }, { &B }, rlk, { &E1 }));
        X(IA, "null ciphertext", cp({ &A, &E1 }), ev.multiply_reduced_error_many({ &A }, { nullptr }, rlk, { &E1 }));
        X(IA, "destinations must be distinct and must not be inputs", cp({ &A, &B }), ev.multiply_reduced_error_many({ &A }, { &B }, rlk, { &A }));
        X(IA, "destinations must be distinct and must not be inputs", cp({ &A, &B }), ev.multiply_reduced_error_many({ &A }, { &B }, rlk, { &B }));
        X(IA, "NTT form mismatch", cp({ &A, &COEFF, &E1 }), ev.multiply_reduced_error_many({ &A }, { &COEFF }, rlk, { &E1 }));
        X(IA, "null ciphertext", cp({ &A }), ev.rescale_to_next_inplace_many({ &A, nullptr }));
        X(IA, "end of modulus switching chain reached", cp({ &A, &LAST, &B }), ev.rescale_to_next_inplace_many({ &A, &LAST, &B }));
        X(IA, "CKKS encrypted must be in NTT form", cp({ &A, &COEFF, &B }), ev.rescale_to_next_inplace_many({ &A, &COEFF, &B }));
        X(IA, "encrypted" + NV, cp({ &A, &EMPTY, &B }), ev.rescale_to_next_inplace_many({ &A, &EMPTY, &B }));
        X(IA, oob(HUGE2.scale() / q_last, low), cp({ &A, &HUGE2, &B }), ev.rescale_to_next_inplace_many({ &A, &HUGE2, &B }));
        std::printf("exception table: %d checks, %d failed\n", g_checks, g_fail);

        // ------------------------------------------------------------------ b. alias matrix
        // inputs one level down, the "larger ciphertext at another level" is the size-3 top-level C3
        Ciphertext x = fresh(low), y = fresh(low), x3, top = fresh(first);
        ev.multiply(x, y, x3);
        Plaintext px = plain(low, S);
        const std::vector<double> vec = values();
        auto unary = [&](const std::string &name, const Ciphertext &in,
                         const std::function<void(const Ciphertext &, Ciphertext &)> &out_fn,
                         const std::function<void(Ciphertext &)> &ip_fn, bool alias = true) {
            Ciphertext want = in, d1, d2 = C3, d3 = in;
            ip_fn(want);
            out_fn(in, d1);
            check(name + ": fresh destination == in-place", same(d1, want));
            out_fn(in, d2);
            check(name + ": destination holding a larger ciphertext == in-place", same(d2, want));
            if (!alias) return; // (apply_galois_to refuses destination == input: exception table)
            out_fn(d3, d3);
            check(name + ": destination == input == in-place", same(d3, want));
        };
        // with destination == b the result is ip(copy of b, a) where swapped (the documented
        // behaviour of the *_reduced_error forms), else ip(copy of a, b)
        auto binary = [&](const std::string &name, const Ciphertext &a, const Ciphertext &b,
                          const std::function<void(const Ciphertext &, const Ciphertext &, Ciphertext &)> &out_fn,
                          const std::function<void(Ciphertext &, const Ciphertext &)> &ip_fn, bool swapped) {
            Ciphertext want = a, wantb = swapped ? b : a, d1, d2 = C3, d3 = a, d4 = b;
            ip_fn(want, b);
            if (swapped)
                ip_fn(wantb, a);
            else
                wantb = want;
            out_fn(a, b, d1);
            check(name + ": fresh destination == in-place", same(d1, want));
            out_fn(a, b, d2);
            check(name + ": destination holding a larger ciphertext == in-place", same(d2, want));
            out_fn(d3, b, d3);
            check(name + ": destination == encrypted1 == in-place", same(d3, want));
            out_fn(a, d4, d4);
            check(name + ": destination == encrypted2 == in-place" + (swapped ? " (operands swapped)" : ""),
                  same(d4, wantb));
        };
        unary("negate", x, [&](const Ciphertext &a, Ciphertext &d) { ev.negate(a, d); },
              [&](Ciphertext &a) { ev.negate_inplace(a); });
        unary("square", x, [&](const Ciphertext &a, Ciphertext &d) { ev.square(a, d); },
              [&](Ciphertext &a) { ev.square_inplace(a); });
        unary("relinearize", x3, [&](const Ciphertext &a, Ciphertext &d) { ev.relinearize(a, rlk, d); },
              [&](Ciphertext &a) { ev.relinearize_inplace(a, rlk); });
        unary("mod_switch_to_next", x, [&](const Ciphertext &a, Ciphertext &d) { ev.mod_switch_to_next(a, d); },
              [&](Ciphertext &a) { ev.mod_switch_to_next_inplace(a); });
        unary("mod_switch_to", x, [&](const Ciphertext &a, Ciphertext &d) { ev.mod_switch_to(a, last, d); },
              [&](Ciphertext &a) { ev.mod_switch_to_inplace(a, last); });
        unary("rescale_to_next", x3, [&](const Ciphertext &a, Ciphertext &d) { ev.rescale_to_next(a, d); },
              [&](Ciphertext &a) { ev.rescale_to_next_inplace(a); });
        unary("multiply_plain", x, [&](const Ciphertext &a, Ciphertext &d) { ev.multiply_plain(a, px, d); },
              [&](Ciphertext &a) { ev.multiply_plain_inplace(a, px); });
        unary("add_plain", x, [&](const Ciphertext &a, Ciphertext &d) { ev.add_plain(a, px, d); },
              [&](Ciphertext &a) { ev.add_plain_inplace(a, px); });
        unary("sub_plain", x, [&](const Ciphertext &a, Ciphertext &d) { ev.sub_plain(a, px, d); },
              [&](Ciphertext &a) { ev.sub_plain_inplace(a, px); });
        unary("apply_galois_to", x, [&](const Ciphertext &a, Ciphertext &d) { ev.apply_galois_to(a, e1, glk, d); },
              [&](Ciphertext &a) { ev.apply_galois_inplace(a, e1, glk); }, false);
        for (int st : { 1, 3, 0, -1 })
            unary("rotate_vector step " + std::to_string(st), x,
                  [&](const Ciphertext &a, Ciphertext &d) { ev.rotate_vector(a, st, glk, d); },
                  [&](Ciphertext &a) { ev.rotate_vector_inplace(a, st, glk); });
        unary("complex_conjugate", x, [&](const Ciphertext &a, Ciphertext &d) { ev.complex_conjugate(a, gconj, d); },
              [&](Ciphertext &a) { ev.complex_conjugate_inplace(a, gconj); });
        unary("add_const", x, [&](const Ciphertext &a, Ciphertext &d) { ev.add_const(a, 0.75, d); },
              [&](Ciphertext &a) { ev.add_const_inplace(a, 0.75); });
        unary("add_const (size 3)", x3, [&](const Ciphertext &a, Ciphertext &d) { ev.add_const(a, 0.75, d); },
              [&](Ciphertext &a) { ev.add_const_inplace(a, 0.75); });
        unary("multiply_const", x, [&](const Ciphertext &a, Ciphertext &d) { ev.multiply_const(a, -1.5, d); },
              [&](Ciphertext &a) { ev.multiply_const_inplace(a, -1.5); });
        unary("multiply_vector", x,
              [&](const Ciphertext &a, Ciphertext &d) { ev.multiply_vector(const_cast<Ciphertext &>(a), vec, d); },
              [&](Ciphertext &a) { ev.multiply_vector_inplace(a, vec); });
        unary("multiply_vector_reduced_error", x,
              [&](const Ciphertext &a, Ciphertext &d) { ev.multiply_vector_reduced_error(const_cast<Ciphertext &>(a), vec, d); },
              [&](Ciphertext &a) { ev.multiply_vector_inplace_reduced_error(a, vec); });
        binary("add", x, y, [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.add(a, b, d); },
               [&](Ciphertext &a, const Ciphertext &b) { ev.add_inplace(a, b); }, false);
        Ciphertext y2 = y;
        y2.scale() = x3.scale();
        binary("add (size 3 + size 2)", x3, y2, [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.add(a, b, d); },
               [&](Ciphertext &a, const Ciphertext &b) { ev.add_inplace(a, b); }, false);
        binary("sub (size 3 - size 2)", x3, y2, [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.sub(a, b, d); },
               [&](Ciphertext &a, const Ciphertext &b) { ev.sub_inplace(a, b); }, false);
        binary("sub", x, y, [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.sub(a, b, d); },
               [&](Ciphertext &a, const Ciphertext &b) { ev.sub_inplace(a, b); }, false);
        binary("multiply", x, y, [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.multiply(a, b, d); },
               [&](Ciphertext &a, const Ciphertext &b) { ev.multiply_inplace(a, b); }, false);
        // reduced-error forms at equal levels (different scales: the result takes encrypted2's) and
        // at unequal levels in both orders
        Ciphertext ys = y;
        ys.scale() = S * 1.25;
        const struct
        {
            const char *tag;
            const Ciphertext *a, *b;
        } pairs[] = { { "equal levels", &x, &ys }, { "encrypted1 higher", &top, &y }, { "encrypted2 higher", &x, &top } };
        for (const auto &p : pairs)
        {
            const std::string t = std::string(" (") + p.tag + ")";
            binary("add_reduced_error" + t, *p.a, *p.b,
                   [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.add_reduced_error(a, b, d); },
                   [&](Ciphertext &a, const Ciphertext &b) { ev.add_inplace_reduced_error(a, b); }, true);
            binary("sub_reduced_error" + t, *p.a, *p.b,
                   [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.sub_reduced_error(a, b, d); },
                   [&](Ciphertext &a, const Ciphertext &b) { ev.sub_inplace_reduced_error(a, b); }, true);
            binary("multiply_reduced_error" + t, *p.a, *p.b,
                   [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) { ev.multiply_reduced_error(a, b, rlk, d); },
                   [&](Ciphertext &a, const Ciphertext &b) { ev.multiply_inplace_reduced_error(a, b, rlk); }, true);
        }
        // rotate_sum (destination may be an input) and multiply_plain_sum (it may not: exception
        // table) have no in-place form: against their definitions, one operation at a time.  Steps
        // { 1, 2, 0 } run as one mhe_rotate_sum, { 1, 3 } (3 has no key) one by one.
        for (const std::vector<int> &st : { std::vector<int>{ 1, 2, 0 }, std::vector<int>{ 1, 3 } })
        {
            const std::string name = "rotate_sum steps " + std::to_string(st.size() == 3 ? 120 : 13);
            auto terms = [&](const Ciphertext &a, const Ciphertext &b) {
                return st.size() == 3 ? CtIn{ &a, &b, &a } : CtIn{ &a, &b };
            };
            Ciphertext want, t, d1, d2 = C3, d3 = x, d4 = y;
            ev.rotate_vector(x, st[0], glk, want);
            ev.rotate_vector(y, st[1], glk, t);
            ev.add_inplace_reduced_error(want, t);
            if (st.size() == 3) ev.add_inplace_reduced_error(want, x);
            ev.rotate_sum(terms(x, y), st, glk, d1);
            check(name + ": fresh destination == rotations folded one by one", same(d1, want));
            ev.rotate_sum(terms(x, y), st, glk, d2);
            check(name + ": destination holding a larger ciphertext", same(d2, want));
            ev.rotate_sum(terms(d3, y), st, glk, d3);
            check(name + ": destination == first input", same(d3, want));
            ev.rotate_sum(terms(x, d4), st, glk, d4);
            check(name + ": destination == second input", same(d4, want));
        }
        {
            Ciphertext want, d1, d2 = C3;
            ev.multiply_plain(x, px, want);
            ev.multiply_plain_add_reduced_error(want, y, px);
            ev.multiply_plain_sum({ &x, &y }, { &px, &px }, d1);
            check("multiply_plain_sum: fresh destination == products added one by one", same(d1, want));
            ev.multiply_plain_sum({ &x, &y }, { &px, &px }, d2);
            check("multiply_plain_sum: destination holding a larger ciphertext", same(d2, want));
        }
        std::printf("alias matrix: %d checks so far, %d failed\n", g_checks, g_fail);

        // ------------------------------------------------------------------ c. launch fingerprint
        struct Inputs
        {
            Ciphertext a, b, la, lb;
            std::vector<Ciphertext> prod; // 9 size-3 products at the top level
            std::vector<Ciphertext> resc; // two (level, size) groups
            Plaintext p, pl;
        };
        auto make_inputs = [&] {
            Inputs in;
            in.a = fresh(first);
            in.b = fresh(first);
            in.la = fresh(low);
            in.lb = fresh(low);
            for (int i = 0; i < 9; i++)
            {
                Ciphertext m;
                ev.multiply(in.a, in.b, m);
                in.prod.push_back(m);
            }
            for (int i = 0; i < 4; i++)
            {
                Ciphertext m;
                if (i < 2)
                    ev.multiply(in.la, in.lb, m); // low level, size 3
                else
                    ev.multiply_const(in.a, 1.0, m); // top level, size 2
                in.resc.push_back(m);
            }
            in.p = plain(first, S);
            in.pl = plain(low, S);
            return in;
        };
        std::uint64_t vec_id = 0;
        auto script = [&](Inputs in, std::uint64_t id) {
            Ciphertext &a = in.a, &b = in.b, &la = in.la, &lb = in.lb;
            Ciphertext d, t, u;
            Plaintext pt;
            ev.negate(a, d);
            ev.negate_inplace(d);
            ev.add(a, b, d);
            ev.add_inplace(d, b);
            ev.add_many({ a, b, a }, d);
            ev.sub(a, b, d);
            ev.sub_inplace(d, b);
            ev.multiply(a, b, d);
            ev.relinearize_inplace(d, rlk);
            ev.rescale_to_next_inplace(d);
            t = a;
            ev.multiply_inplace(t, b);
            ev.relinearize(t, rlk, d);
            ev.rescale_to_next(d, u);
            ev.square(a, d);
            t = la;
            ev.square_inplace(t);
            ev.rescale_to_inplace(t, last);
            ev.mod_switch_to_next(a, d);
            t = a;
            ev.mod_switch_to_next_inplace(t);
            ev.mod_switch_to(a, last, d);
            t = a;
            ev.mod_switch_to_inplace(t, low);
            pt = in.p;
            ev.mod_switch_to_next_inplace(pt);
            pt = in.p;
            ev.mod_switch_to_inplace(pt, last);
            ev.multiply_plain(a, in.p, d);
            t = la;
            ev.multiply_plain_inplace(t, in.pl);
            ev.add_plain(a, in.p, d);
            ev.add_plain_inplace(d, in.p);
            ev.sub_plain(a, in.p, d);
            ev.sub_plain_inplace(d, in.p);
            t = a;
            ev.transform_from_ntt_inplace(t);
            ev.transform_to_ntt_inplace(t);
            t = a;
            ev.apply_galois_inplace(t, e1, glk);
            ev.apply_galois_to(la, e1, glk, d);
            t = a;
            ev.rotate_vector_inplace(t, 2, glk);
            ev.rotate_vector_inplace(t, 3, glk);
            ev.rotate_vector(a, 4, glk, d);
            ev.rotate_vector(a, 0, glk, d);
            ev.rotate_vector(la, 3, glk, d);
            t = a;
            ev.complex_conjugate_inplace(t, gconj);
            ev.complex_conjugate(la, gconj, d);
            ev.add_const(a, 0.5, d);
            ev.add_const_inplace(d, 0.25);
            ev.multiply_const(a, 0.5, d);
            t = la;
            ev.multiply_const_inplace(t, 2.0);
            t = a;
            ev.multiply_vector_inplace(t, vec);
            ev.multiply_vector(a, vec, d);
            ev.multiply_vector_reduced_error(la, vec, d);
            ev.encode_vector_for(la, vec, pt);
            ev.cached_vector_plain(a, 77, id, [&] { return vec; }, pt);
            t = a;
            ev.add_inplace_reduced_error(t, b);
            ev.add_inplace_reduced_error(t, lb);
            ev.add_reduced_error(a, b, d);
            ev.add_reduced_error(la, b, d);
            t = a;
            ev.sub_inplace_reduced_error(t, b);
            ev.sub_reduced_error(a, b, d);
            ev.sub_reduced_error(a, lb, d);
            t = a;
            ev.multiply_inplace_reduced_error(t, b, rlk);
            ev.multiply_reduced_error(a, b, rlk, d);
            ev.multiply_reduced_error(la, b, rlk, d);
            ev.multiply_reduced_error(a, lb, rlk, d);
            ev.multiply_plain(a, in.p, t);
            ev.multiply_plain_add_reduced_error(t, b, in.p);
            ev.multiply_plain_sum({ &a, &b, &a }, { &in.p, &in.p, &in.p }, d);
            // the batched mixes
            std::vector<Ciphertext> r(5);
            ev.rotate_vectors({ &a, &b, &la, &a, &b }, { 1, 2, 1, 0, 3 }, glk, { &r[0], &r[1], &r[2], &r[3], &r[4] });
            ev.rotate_sum({ &a, &b, &a }, { 1, 2, 0 }, glk, d);
            ev.rotate_sum({ &a, &lb }, { 1, 2 }, glk, d);
            CtOut pp;
            for (auto &c : in.prod) pp.push_back(&c);
            ev.relinearize_inplace_many(pp, rlk);
            CtOut pr;
            for (auto &c : in.resc) pr.push_back(&c);
            ev.rescale_to_next_inplace_many(pr);
            std::vector<Ciphertext> m(3);
            ev.multiply_reduced_error_many({ &a, &la, &a }, { &b, &lb, &lb }, rlk, { &m[0], &m[1], &m[2] });
        };
        std::vector<Inputs> members;
        for (int m = 0; m < 3; m++) members.push_back(make_inputs());
        auto reset_counts = [&] {
            std::uint64_t c[8];
            for (int k = 0; k < 8; k++) mhe_op_counts(ctx.engine(), k, c, 8, 1);
            merged_call_fallbacks(true);
        };
        auto counts = [&] {
            std::string s;
            for (int k = 0; k < 8; k++)
            {
                std::uint64_t c[8] = { 0 };
                mhe_op_counts(ctx.engine(), k, c, 8, 0);
                s += "k" + std::to_string(k) + ":";
                for (int l = 0; l < 8; l++) s += " " + std::to_string(c[l]);
                s += "; ";
            }
            return s;
        };
        // the parent commit's numbers (deterministic; zero margin)
        const std::string want_direct =
            "k0: 0 0 0 0 10 27 0 0; "
            "k1: 0 0 3 3 9 22 0 0; "
            "k2: 0 0 0 0 5 6 0 0; "
            "k3: 0 0 0 0 4 16 0 0; "
            "k4: 0 0 0 0 8 38 0 0; "
            "k5: 0 0 0 0 2 18 0 0; "
            "k6: 0 0 0 0 2 7 0 0; "
            "k7: 0 0 0 0 12 26 0 0; "
            "fallbacks 0";
        const std::string want_fibers =
            "k0: 0 0 0 0 30 81 0 0; "
            "k1: 0 0 9 9 27 66 0 0; "
            "k2: 0 0 0 0 15 18 0 0; "
            "k3: 0 0 0 0 12 48 0 0; "
            "k4: 0 0 0 0 24 114 0 0; "
            "k5: 0 0 0 0 6 54 0 0; "
            "k6: 0 0 0 0 6 21 0 0; "
            "k7: 0 0 0 0 36 78 0 0; "
            "fiber rounds 127 merged 381; "
            "fallbacks 0";
        const std::string want_lockstep =
            "k0: 0 0 0 0 30 81 0 0; "
            "k1: 0 0 9 9 27 66 0 0; "
            "k2: 0 0 0 0 15 18 0 0; "
            "k3: 0 0 0 0 12 48 0 0; "
            "k4: 0 0 0 0 24 114 0 0; "
            "k5: 0 0 0 0 6 54 0 0; "
            "k6: 0 0 0 0 6 21 0 0; "
            "k7: 0 0 0 0 36 78 0 0; "
            "lockstep rounds 20 merged 60; "
            "fallbacks 0";

        reset_counts();
        script(members[0], vec_id++);
        const std::string got_direct = counts() + "fallbacks " + std::to_string(merged_call_fallbacks());
        std::printf("fingerprint direct:   %s\n", got_direct.c_str());
        check("launch fingerprint, direct", got_direct == want_direct);

        reset_counts();
        FiberBatch::run(3, [&](std::size_t m) { script(members[m], 16 + m); });
        const std::string got_fibers = counts() + "fiber rounds " + std::to_string(FiberBatch::last_rounds()) + " merged " +
                                       std::to_string(FiberBatch::last_merged()) + "; fallbacks " +
                                       std::to_string(merged_call_fallbacks());
        std::printf("fingerprint fibers:   %s\n", got_fibers.c_str());
        check("launch fingerprint, FiberBatch of 3", got_fibers == want_fibers);

        reset_counts();
        Lockstep group(3);
        {
            std::vector<std::thread> th;
            for (int m = 0; m < 3; m++)
                th.emplace_back([&, m] {
                    Lockstep::Member member(group);
                    script(members[m], 32 + m);
                });
            for (auto &t : th) t.join();
        }
        const std::string got_lockstep = counts() + "lockstep rounds " + std::to_string(group.rounds()) + " merged " +
                                         std::to_string(group.merged_calls()) + "; fallbacks " +
                                         std::to_string(merged_call_fallbacks());
        std::printf("fingerprint lockstep: %s\n", got_lockstep.c_str());
        check("launch fingerprint, Lockstep group of 3", got_lockstep == want_lockstep);
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\nFAILED\n", e.what());
        return 1;
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    std::printf(g_fail ? "FAILED\n" : "ALL PASSED\n");
    return g_fail ? 1 : 0;
}
