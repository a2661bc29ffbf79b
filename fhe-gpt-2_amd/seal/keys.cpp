// keys.cpp -- KSwitchKeys (with the deferred, level-truncated Galois keys) and KeyGenerator
// (keygenerator.cpp, rlwe.cpp encrypt_zero_symmetric).
#include "seal_internal.h"
#include "random_internal.h"

#include <algorithm>
#include <functional>
#include <map>
#include <mutex>

namespace seal
{
// ------------------------------------------------------------------------------ KeyGenerator
// keygenerator.cpp: secret key (sparse ternary with the modified hamming weight, else ternary)
// in NTT form at the key level; public key and key-switching keys are symmetric encryptions of
// zero at the key level (rlwe.cpp encrypt_zero_symmetric), the latter with
// (P mod q_i) * s'_i added to digit i's limb i (keygenerator.cpp:384-414).
static void upload(mhe_ctx *eng, void *s, std::uint64_t *dst, const std::vector<std::uint64_t> &h)
{
    chk(mhe_memcpy_h2d(eng, dst, h.data(), h.size() * 8, s));
    chk(mhe_stream_sync(eng, s)); // the host vector is temporary
}

// encrypt_zero_symmetric (rlwe.cpp:289-373) at a level of `limbs` primes, NTT form, no seed
// saved: bootstrap PRNG <- `seed`; its first 64 bytes seed the PRNG of a = c1 (sample_poly_uniform,
// NTT form directly); e = sample_poly_cbd from the bootstrap PRNG's next bytes; c0 = -(a*s + e).
void sym_encrypt_zero(const SEALContext &ctx, const prng_seed_type &seed, const std::uint64_t *sk,
                            std::size_t limbs, std::uint64_t *c0, std::uint64_t *c1, void *s)
{
    mhe_ctx *eng = ctx.engine();
    const std::size_t n = ctx.key_context_data()->parms().poly_modulus_degree();
    rnd::sample_uniform_dev(eng, rnd::stream_prefix_seed(seed), moduli_of(ctx), limbs, n, c1, s);
    rnd::sample_cbd_dev(eng, seed, prng_seed_byte_count, limbs, c0, s);
    chk(mhe_ntt_forward(eng, c0, 1, (int)limbs, 0, s));
    DevBuf t(eng, s, limbs * n);
    chk(mhe_multiply_plain(eng, sk, c1, t.p, 1, (int)limbs, s));
    chk(mhe_add(eng, t.p, c0, c0, 1, (int)limbs, s));
    chk(mhe_negate(eng, c0, c0, 1, (int)limbs, s));
}

namespace
{
// generate_one_kswitch_key (keygenerator.cpp:384-414) truncated to `digits` digits: digit j is an
// encryption of zero over the key level (its own bootstrap seed, next_seed()) with
// (P mod q_j) * new_key added to limb j of c0; the stored key keeps primes q_0..q_{digits-1} and
// P ([digits][2][digits+1][n]).  digits = K-1 is SEAL's full key; a truncated key is SEAL's key
// restricted to those digits and primes.
//
// The opening of both ways to make it: the checks, and the store sized and ready to be overwritten.
std::uint64_t *kswitch_key_store(const SEALContext &ctx, std::size_t digits, PolyStore &dest)
{
    const std::size_t K = ctx.key_size(), n = ctx.key_context_data()->parms().poly_modulus_degree();
    if (K < 2) throw std::logic_error("keyswitching is not supported by the context");
    if (digits < 1 || digits > K - 1) throw std::invalid_argument("key digits out of range");
    dest.bind(ctx);
    dest.resize_words(digits * 2 * (digits + 1) * n, false);
    return dest.dev_write(ctx.stream(), true);
}

// The per-digit sequence of general-purpose calls (the whole digit is drawn over the key level, then
// the kept limbs copied): the path with batched launches off, and the redo of a key whose uniform
// sampler overflowed its redraw buffer.
void make_kswitch_key_seq(const SEALContext &ctx, const std::function<prng_seed_type()> &next_seed,
                          const std::uint64_t *sk, const std::uint64_t *new_key, std::size_t digits, PolyStore &dest)
{
    std::uint64_t *d = kswitch_key_store(ctx, digits, dest);
    const std::size_t K = ctx.key_size(), n = ctx.key_context_data()->parms().poly_modulus_degree();
    const auto &cm = ctx.key_context_data()->parms().coeff_modulus();
    mhe_ctx *eng = ctx.engine();
    void *s = ctx.stream();
    const std::size_t KL = digits + 1; // stored limbs
    DevBuf t(eng, s, K * n);
    const bool full = KL == K;
    DevBuf tmp(eng, s, full ? 1 : 2 * K * n);
    const std::uint64_t P = cm[K - 1].value();
    for (std::size_t j = 0; j < digits; j++)
    {
        std::uint64_t *c0 = full ? d + j * 2 * K * n : tmp.p, *c1 = c0 + K * n;
        sym_encrypt_zero(ctx, next_seed(), sk, K, c0, c1, s);
        std::vector<std::uint64_t> f(K, 0);
        f[j] = P % cm[j].value();
        chk(mhe_multiply_scalar(eng, new_key, f.data(), t.p, 1, (int)K, s));
        chk(mhe_add(eng, c0, t.p, c0, 1, (int)K, s));
        if (!full)
            for (int c = 0; c < 2; c++)
            {
                const std::uint64_t *src = tmp.p + c * K * n;
                std::uint64_t *dst = d + (j * 2 + c) * KL * n;
                chk(mhe_memcpy_d2d(eng, dst, src, digits * n * 8, s));
                chk(mhe_memcpy_d2d(eng, dst + digits * n, src + (K - 1) * n, n * 8, s));
            }
    }
}

// The same key from one mhe_encrypt_sk_batch over all digits, written straight into the destination
// store: the seeds are drawn in digit order on the host, nothing synchronises.  `drawn` receives the
// bootstrap seeds, with which a caller redoes the key by make_kswitch_key_seq when the engine reports
// an overflow at the end of its create_* call (redo_if_overflowed).
void make_kswitch_key(const SEALContext &ctx, const std::function<prng_seed_type()> &next_seed,
                      const std::uint64_t *sk, const std::uint64_t *new_key, std::size_t digits, PolyStore &dest,
                      std::vector<prng_seed_type> *drawn = nullptr)
{
    if (!batched_launches() || trace::enabled()) return make_kswitch_key_seq(ctx, next_seed, sk, new_key, digits, dest);
    std::uint64_t *d = kswitch_key_store(ctx, digits, dest);
    const std::size_t K = ctx.key_size(), n = ctx.key_context_data()->parms().poly_modulus_degree();
    const std::size_t KL = digits + 1; // stored limbs
    std::vector<prng_seed_type> seeds(digits);
    std::vector<const std::uint64_t *> nk(digits, new_key);
    std::vector<int> dg(digits);
    std::vector<std::uint64_t *> outs(digits);
    for (std::size_t j = 0; j < digits; j++)
    {
        seeds[j] = next_seed();
        dg[j] = (int)j;
        outs[j] = d + j * 2 * KL * n;
    }
    chk(mhe_encrypt_sk_batch(ctx.engine(), (int)digits, reinterpret_cast<const std::uint64_t(*)[8]>(seeds.data()), sk,
                             (int)K, (int)digits, 1, nk.data(), dg.data(), outs.data(), ctx.stream()));
    if (drawn) *drawn = std::move(seeds);
}

// The new key that the key-switching key of Galois element `elt` switches from, over the key level
// into nk: s(X^elt) (apply_galois_ntt on the NTT-form secret key), or s * s for elt = 0, the
// relinearization key.
void new_key_of(const SEALContext &ctx, const std::uint64_t *sk, std::uint32_t elt, std::uint64_t *nk)
{
    if (elt)
        chk(mhe_permute_galois(ctx.engine(), sk, elt, nk, 1, (int)ctx.key_size(), ctx.stream()));
    else
        chk(mhe_multiply_plain(ctx.engine(), sk, sk, nk, 1, (int)ctx.key_size(), ctx.stream()));
}

// A function that hands out `seeds` in order (the replay of a key's draws).
std::function<prng_seed_type()> replay(const std::vector<prng_seed_type> &seeds)
{
    auto i = std::make_shared<std::size_t>(0);
    return [&seeds, i] { return seeds.at((*i)++); };
}

// The one synchronisation of a create_* call that took the batched path: true when a key it made may
// hold words of an overflowed redraw buffer and has to be redone.
bool overflowed(const SEALContext &ctx)
{
    return batched_launches() && !trace::enabled() && rnd::uniform_overflow_moved(ctx.engine(), ctx.stream());
}
} // namespace

// Deferred Galois keys (see seal.h, KeyGenerator::create_deferred_galois_keys): a client-side key
// provider holding the secret key and, per key index, its Galois element and a 512-bit seed.
// Digit j of a materialised key draws its bootstrap seed from bytes [64j, 64j+64) of that seed's
// stream, so a key re-materialised larger keeps its smaller prefix.
struct KeyMaker
{
    std::mutex mu;
    SEALContext ctx;
    PolyStore sk; // NTT form over the key level
    std::map<std::size_t, std::pair<std::uint32_t, prng_seed_type>> elts;
    explicit KeyMaker(const SEALContext &c) : ctx(c) {}
};

std::size_t KSwitchKeys::size() const
{
    if (!maker_) return keys_.size();
    std::lock_guard<std::mutex> lk(maker_->mu);
    std::size_t c = maker_->elts.size();
    for (const auto &kv : keys_)
        if (!maker_->elts.count(kv.first)) c++;
    return c;
}

bool KSwitchKeys::has_index(std::size_t i) const
{
    if (maker_)
    {
        std::lock_guard<std::mutex> lk(maker_->mu);
        if (maker_->elts.count(i)) return true;
    }
    return keys_.count(i) != 0;
}

const PolyStore &KSwitchKeys::key(std::size_t i) const
{
    auto it = keys_.find(i);
    if (it == keys_.end()) throw std::out_of_range("kswitch_keys_index");
    return it->second;
}

std::size_t KSwitchKeys::limbs_of(std::size_t i) const
{
    auto it = limbs_of_.find(i);
    return it == limbs_of_.end() ? key_limbs_ : it->second;
}

const std::uint64_t *KSwitchKeys::key_for(std::size_t i, std::size_t L, void *stream, std::size_t &key_limbs) const
{
    if (maker_)
    {
        std::lock_guard<std::mutex> lk(maker_->mu);
        auto e = maker_->elts.find(i);
        if (e != maker_->elts.end())
        {
            auto lt = limbs_of_.find(i);
            if (lt == limbs_of_.end() || lt->second < L + 1)
            {
                // materialise (or grow) the level-truncated key on the maker's context stream
                const SEALContext &ctx = maker_->ctx;
                const std::size_t K = ctx.key_size();
                const std::size_t digits = std::min(K - 1, std::max<std::size_t>(L, 1));
                void *s = ctx.stream();
                const std::size_t n = ctx.key_context_data()->parms().poly_modulus_degree();
                DevBuf rot(ctx.engine(), s, K * n);
                const std::uint64_t *sk = maker_->sk.dev_read(s);
                new_key_of(ctx, sk, e->second.first, rot.p);
                Blake2xbPRNG seeds(e->second.second);
                PolyStore fresh;
                std::vector<prng_seed_type> drawn;
                make_kswitch_key(
                    ctx,
                    [&] {
                        prng_seed_type d;
                        seeds.generate(prng_seed_byte_count, reinterpret_cast<seal_byte *>(d.data()));
                        return d;
                    },
                    sk, rot.p, digits, fresh, &drawn);
                if (!drawn.empty() && overflowed(ctx)) make_kswitch_key_seq(ctx, replay(drawn), sk, rot.p, digits, fresh);
                auto kt = keys_.find(i);
                if (kt != keys_.end()) retired_.push_back(std::move(kt->second));
                keys_[i] = std::move(fresh);
                limbs_of_[i] = digits + 1;
            }
            key_limbs = limbs_of_[i];
            return keys_.find(i)->second.dev_read(stream);
        }
    }
    key_limbs = limbs_of(i);
    if (key_limbs < L + 1)
        throw std::invalid_argument("key-switching key is truncated below the ciphertext level");
    return key(i).dev_read(stream);
}

std::map<std::size_t, std::size_t> KSwitchKeys::usage() const
{
    std::map<std::size_t, std::size_t> u;
    for (const auto &kv : keys_) u[kv.first] = limbs_of(kv.first);
    return u;
}

std::size_t KSwitchKeys::device_bytes() const
{
    std::size_t b = 0;
    for (const auto &kv : keys_) b += kv.second.words() * 8;
    for (const auto &r : retired_) b += r.words() * 8;
    return b;
}

void KSwitchKeys::insert(std::size_t index, PolyStore &&key, std::size_t limbs)
{
    keys_[index] = std::move(key);
    limbs_of_[index] = limbs;
}

KeyGenerator::KeyGenerator(const SEALContext &context) : ctx_(context)
{
    require_set(context);
    // keygenerator.cpp:62-84: the secret key from a fresh PRNG of the parameters' factory,
    // sparse ternary with the modified Hamming weight (or ternary for weight 0), NTT form
    const auto &parms = context.key_context_data()->parms();
    rng_ = factory_of(context);
    const std::size_t K = context.key_size(), n = parms.poly_modulus_degree();
    const std::size_t hw = parms.secret_key_hamming_weight();
    const auto q = moduli_of(context);
    std::vector<std::uint64_t> h(K * n);
    {
        auto prng = rng_->create();
        if (hw)
            rnd::sample_sparse_ternary_host(*prng, q, n, hw, h.data());
        else
            rnd::sample_ternary_host(*prng, q, K, n, h.data());
    }
    void *s = context.stream();
    sk_.data().set_level(context, context.key_parms_id(), K);
    std::uint64_t *d = sk_.data().store().dev_write(s, true);
    upload(context.engine(), s, d, h);
    std::fill(h.begin(), h.end(), 0);
    chk(mhe_ntt_forward(context.engine(), d, 1, (int)K, 0, s));
}

KeyGenerator::KeyGenerator(const SEALContext &context, const SecretKey &secret_key) : ctx_(context), sk_(secret_key)
{
    require_set(context);
    if (secret_key.parms_id() != context.key_parms_id())
        throw std::invalid_argument("secret key is not valid for encryption parameters");
    rng_ = factory_of(context);
}

namespace
{
// generate_pk (keygenerator.cpp:87-112): encrypt_zero_symmetric at the key level
prng_seed_type make_public_key(const SEALContext &ctx, UniformRandomGeneratorFactory &rng, const SecretKey &sk,
                               PublicKey &destination)
{
    const std::size_t K = ctx.key_size(), n = ctx.key_context_data()->parms().poly_modulus_degree();
    void *s = ctx.stream();
    Ciphertext &pk = destination.data();
    pk.resize(ctx, ctx.key_parms_id(), 2);
    pk.is_ntt_form() = true;
    pk.scale() = 1.0;
    std::uint64_t *d = pk.store().dev_write(s, true);
    const prng_seed_type seed = rng.next_seed();
    const std::uint64_t *skp = sk.data().store().dev_read(s);
    bool batched = batched_launches() && !trace::enabled();
    if (batched)
    {
        // one entry, every limb of the key level kept: [2][K][n] is the public key's own layout
        chk(mhe_encrypt_sk_batch(ctx.engine(), 1, reinterpret_cast<const std::uint64_t(*)[8]>(seed.data()), skp, (int)K,
                                 (int)K, 0, nullptr, nullptr, &d, s));
        batched = !overflowed(ctx);
    }
    if (!batched) sym_encrypt_zero(ctx, seed, skp, K, d, d + K * n, s);
    return rnd::stream_prefix_seed(seed);
}
} // namespace

void KeyGenerator::create_public_key(PublicKey &destination) { make_public_key(ctx_, *rng_, sk_, destination); }

Serializable<PublicKey> KeyGenerator::create_public_key()
{
    PublicKey pk;
    const prng_seed_type seed = make_public_key(ctx_, *rng_, sk_, pk);
    return Serializable<PublicKey>(std::move(pk), SeedMap{ { 0, { seed } } });
}

// One key of a create_* call: its new key into nk (K * n words), the key-switching key from this
// generator's next seeds, inserted at m.index.  A key that came from the batched launches is
// remembered in `made` with its bootstrap seeds; none is when the per-digit sequence ran.
void KeyGenerator::make_key(KSwitchKeys &destination, MadeKey m, SeedMap *seeds, std::uint64_t *nk,
                            std::vector<MadeKey> &made)
{
    const std::uint64_t *sk = sk_.data().store().dev_read(ctx_.stream());
    new_key_of(ctx_, sk, m.elt, nk);
    std::vector<prng_seed_type> *pub = seeds ? &(*seeds)[m.index] : nullptr;
    PolyStore key;
    make_kswitch_key(
        ctx_,
        [&] {
            const prng_seed_type sd = rng_->next_seed();
            if (pub) pub->push_back(rnd::stream_prefix_seed(sd));
            return sd;
        },
        sk, nk, m.digits, key, &m.seeds);
    destination.insert(m.index, std::move(key), m.digits + 1);
    if (!m.seeds.empty()) made.push_back(std::move(m));
}

// The end of a create_* call: when the engine reports an overflowed redraw buffer, every key the call
// made by the batched path is made again from its seeds by the per-digit sequence and replaces the
// batched one.
void KeyGenerator::redo_if_overflowed(KSwitchKeys &destination, const std::vector<MadeKey> &made)
{
    if (made.empty() || !overflowed(ctx_)) return;
    const std::size_t K = ctx_.key_size(), n = ctx_.key_context_data()->parms().poly_modulus_degree();
    void *s = ctx_.stream();
    DevBuf nk(ctx_.engine(), s, K * n);
    const std::uint64_t *sk = sk_.data().store().dev_read(s);
    for (const MadeKey &m : made)
    {
        new_key_of(ctx_, sk, m.elt, nk.p);
        PolyStore key;
        make_kswitch_key_seq(ctx_, replay(m.seeds), sk, nk.p, m.digits, key);
        destination.insert(m.index, std::move(key), m.digits + 1);
    }
}

void KeyGenerator::create_relin_keys(RelinKeys &destination) { relin_keys_into(destination, nullptr); }

Serializable<RelinKeys> KeyGenerator::create_relin_keys()
{
    RelinKeys rk;
    SeedMap seeds;
    relin_keys_into(rk, &seeds);
    return Serializable<RelinKeys>(std::move(rk), std::move(seeds));
}

void KeyGenerator::relin_keys_into(RelinKeys &destination, SeedMap *seeds)
{
    // create_relin_keys (keygenerator.cpp:115-149): key-switching key of s^2
    const std::size_t K = ctx_.key_size(), n = ctx_.key_context_data()->parms().poly_modulus_degree();
    DevBuf s2(ctx_.engine(), ctx_.stream(), K * n);
    std::vector<MadeKey> made;
    make_key(destination, MadeKey{ RelinKeys::get_index(2), 0, K - 1, {} }, seeds, s2.p, made);
    redo_if_overflowed(destination, made);
    destination.parms_id() = ctx_.key_parms_id();
    destination.set_key_limbs(K);
}

// SEAL's full keys: every element at more limbs than any level has
static std::vector<std::pair<std::uint32_t, std::size_t>> full_keys(const std::vector<std::uint32_t> &elts)
{
    std::vector<std::pair<std::uint32_t, std::size_t>> el;
    for (std::uint32_t elt : elts) el.emplace_back(elt, ~std::size_t(0));
    return el;
}

void KeyGenerator::create_galois_keys(const std::vector<std::pair<std::uint32_t, std::size_t>> &elt_limbs,
                                      GaloisKeys &destination)
{
    galois_keys_into(elt_limbs, destination, nullptr);
}

void KeyGenerator::create_galois_keys_from_elts(const std::vector<std::uint32_t> &elts, GaloisKeys &destination)
{
    galois_keys_into(full_keys(elts), destination, nullptr);
}

void KeyGenerator::galois_keys_into(const std::vector<std::pair<std::uint32_t, std::size_t>> &elt_limbs,
                                    GaloisKeys &destination, SeedMap *seeds)
{
    // create_galois_keys (keygenerator.cpp:152-190): per element, the key-switching key of s(X^elt),
    // here truncated per element to the level it is used at (limbs = ciphertext limbs; >= K-1 keeps
    // SEAL's full key); seeds receives every digit's public seed per key index
    const std::size_t K = ctx_.key_size(), n = ctx_.key_context_data()->parms().poly_modulus_degree();
    if (K < 2) throw std::logic_error("keyswitching is not supported by the context");
    DevBuf rot(ctx_.engine(), ctx_.stream(), K * n);
    std::vector<MadeKey> made;
    for (const auto &el : elt_limbs)
    {
        const std::uint32_t elt = el.first;
        if (!(elt & 1) || elt >= 2 * n) throw std::invalid_argument("Galois element is not valid");
        if (destination.has_key(elt)) continue;
        const std::size_t digits = std::min(K - 1, std::max<std::size_t>(el.second, 1));
        make_key(destination, MadeKey{ GaloisKeys::get_index(elt), elt, digits, {} }, seeds, rot.p, made);
    }
    redo_if_overflowed(destination, made);
    destination.parms_id() = ctx_.key_parms_id();
    destination.set_key_limbs(K);
}

void KeyGenerator::create_deferred_galois_keys_from_elts(const std::vector<std::uint32_t> &elts, GaloisKeys &destination)
{
    const std::size_t K = ctx_.key_size(), n = ctx_.key_context_data()->parms().poly_modulus_degree();
    if (K < 2) throw std::logic_error("keyswitching is not supported by the context");
    auto maker = destination.maker();
    if (!maker)
    {
        maker = std::make_shared<KeyMaker>(ctx_);
        maker->sk = sk_.data().store();
        destination.set_maker(maker);
    }
    std::lock_guard<std::mutex> lk(maker->mu);
    for (std::uint32_t elt : elts)
    {
        if (!(elt & 1) || elt >= 2 * n) throw std::invalid_argument("Galois element is not valid");
        const std::size_t idx = GaloisKeys::get_index(elt);
        if (!maker->elts.count(idx)) maker->elts[idx] = { elt, rng_->next_seed() };
    }
    destination.parms_id() = ctx_.key_parms_id();
    destination.set_key_limbs(K);
}

namespace
{
std::vector<std::uint32_t> elts_from_steps(const SEALContext &ctx, const std::vector<int> &steps)
{
    // GaloisTool::get_elts_from_steps (util/galois.cpp:96-104)
    const int log_n = __builtin_ctzll(ctx.key_context_data()->parms().poly_modulus_degree());
    std::vector<std::uint32_t> elts;
    for (int st : steps)
    {
        const std::uint32_t e = mhe_galois_elt_from_step(log_n, st);
        if (!e) throw std::invalid_argument("step count too large");
        elts.push_back(e);
    }
    return elts;
}

std::vector<std::uint32_t> elts_all(const SEALContext &ctx)
{
    // GaloisTool::get_elts_all (util/galois.cpp:106-131), generator 5
    const std::size_t n = ctx.key_context_data()->parms().poly_modulus_degree();
    const std::uint64_t m = 2 * n;
    const int log_n = __builtin_ctzll(n);
    std::vector<std::uint32_t> elts{ (std::uint32_t)(m - 1) };
    std::uint64_t pos = 5, neg = 1;
    // inverse of 5 mod m (m a power of two): 5^(m/4 - 1)
    for (std::uint64_t k = 0; k < m / 4 - 1; k++) neg = (neg * 5) & (m - 1);
    for (int i = 0; i < log_n - 1; i++)
    {
        elts.push_back((std::uint32_t)pos);
        pos = (pos * pos) & (m - 1);
        elts.push_back((std::uint32_t)neg);
        neg = (neg * neg) & (m - 1);
    }
    return elts;
}
} // namespace

void KeyGenerator::create_galois_keys(const std::vector<int> &steps, GaloisKeys &destination)
{
    create_galois_keys_from_elts(elts_from_steps(ctx_, steps), destination);
}

void KeyGenerator::create_galois_keys(GaloisKeys &destination)
{
    create_galois_keys_from_elts(elts_all(ctx_), destination);
}

Serializable<GaloisKeys> KeyGenerator::create_galois_keys(const std::vector<int> &steps)
{
    GaloisKeys gk;
    SeedMap seeds;
    galois_keys_into(full_keys(elts_from_steps(ctx_, steps)), gk, &seeds);
    return Serializable<GaloisKeys>(std::move(gk), std::move(seeds));
}

Serializable<GaloisKeys> KeyGenerator::create_galois_keys()
{
    GaloisKeys gk;
    SeedMap seeds;
    galois_keys_into(full_keys(elts_all(ctx_)), gk, &seeds);
    return Serializable<GaloisKeys>(std::move(gk), std::move(seeds));
}

void KeyGenerator::create_deferred_galois_keys(const std::vector<int> &steps, GaloisKeys &destination)
{
    create_deferred_galois_keys_from_elts(elts_from_steps(ctx_, steps), destination);
}

void KeyGenerator::create_deferred_galois_keys(GaloisKeys &destination)
{
    create_deferred_galois_keys_from_elts(elts_all(ctx_), destination);
}

const GaloisKeys &KeyGenerator::power_of_two_keys()
{
    std::lock_guard<std::mutex> lk(*pow2_mu_);
    if (!pow2_)
    {
        const int log_n = __builtin_ctzll(ctx_.key_context_data()->parms().poly_modulus_degree());
        std::vector<int> steps;
        for (int i = 0; i < log_n - 1; i++)
        {
            steps.push_back(1 << i);
            steps.push_back(-(1 << i));
        }
        pow2_ = std::make_shared<GaloisKeys>();
        create_deferred_galois_keys(steps, *pow2_);
    }
    return *pow2_;
}
} // namespace seal
