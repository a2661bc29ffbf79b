// crypt.cpp -- CKKSEncoder (ckks.h/ckks.cpp), Encryptor (encryptor.cpp:88-239) and Decryptor
// (decryptor.cpp ckks_decrypt).
#include "seal_internal.h"
#include "random_internal.h"

#include <complex>

namespace seal
{
// ------------------------------------------------------------------------------ CKKSEncoder
CKKSEncoder::CKKSEncoder(const SEALContext &context) : ctx_(context)
{
    require_set(context);
    const auto &parms = context.first_context_data()->parms();
    const std::size_t n = parms.poly_modulus_degree();
    slots_ = n >> 1;
    sparse_slots_ = parms.sparse_slots() ? parms.sparse_slots() : slots_;
    chk(mhe_encoder_create(&enc_, __builtin_ctzll(n)));
}

CKKSEncoder::~CKKSEncoder()
{
    if (enc_) (void)mhe_encoder_destroy(enc_);
}

void CKKSEncoder::encode_internal(const double *re, const double *im, std::size_t count, parms_id_type parms_id,
                                  double scale, Plaintext &destination)
{
    auto cd = ctx_.get_context_data(parms_id);
    if (!cd) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    const std::size_t L = cd->parms().coeff_modulus().size();
    if (count > slots_) throw std::invalid_argument("values_size is too large");
    void *s = ctx_.stream();
    destination.set_level(ctx_, parms_id, L);
    destination.scale() = scale;
    chk(mhe_ckks_encode(ctx_.engine(), enc_, re, im, count, scale, (int)L, destination.store().dev_write(s, true),
                        s));
}

void CKKSEncoder::encode(const std::vector<double> &values, parms_id_type parms_id, double scale,
                         Plaintext &destination, MemoryPoolHandle)
{
    TRACE_OP("encode", trace::pt(destination), trace::vec(values.data(), nullptr, values.size()));
    TRACE_EXTRA("\"scale\": " + trace::num(scale));
    encode_internal(values.data(), nullptr, values.size(), parms_id, scale, destination);
}

void CKKSEncoder::encode(const std::vector<std::complex<double>> &values, parms_id_type parms_id, double scale,
                         Plaintext &destination, MemoryPoolHandle)
{
    std::vector<double> re(values.size()), im(values.size());
    for (std::size_t i = 0; i < values.size(); i++)
    {
        re[i] = values[i].real();
        im[i] = values[i].imag();
    }
    TRACE_OP("encode", trace::pt(destination), trace::vec(re.data(), im.data(), re.size()));
    TRACE_EXTRA("\"scale\": " + trace::num(scale));
    encode_internal(re.data(), im.data(), values.size(), parms_id, scale, destination);
}

// data[b]: `count` reals, or with is_complex `count` (re, im) pairs, of entry b
void CKKSEncoder::encode_many_internal(const std::vector<const double *> &data, std::size_t count, bool is_complex,
                                       parms_id_type parms_id, double scale,
                                       const std::vector<Plaintext *> &destinations)
{
    auto cd = ctx_.get_context_data(parms_id);
    if (!cd) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    const std::size_t L = cd->parms().coeff_modulus().size(), B = data.size(), per = count * (is_complex ? 2 : 1);
    if (count > slots_) throw std::invalid_argument("values_size is too large");
    mhe_ctx *eng = ctx_.engine();
    void *s = ctx_.stream();
    // one upload of all the values; the host's l1 norms settle the size check of ordinary inputs, and
    // the status words are read back only when some bound does not prove it
    std::vector<double> host(B * per), l1(B, 0.0);
    for (std::size_t b = 0; b < B; b++)
        for (std::size_t i = 0; i < per; i++) l1[b] += std::fabs(host[b * per + i] = data[b][i]);
    bool checked = false;
    for (std::size_t b = 0; b < B && !checked; b++)
        checked = mhe_ckks_encode_l1_proves(eng, scale, (int)L, l1[b]) != 1;
    DevBuf staging(eng, s, host.size() + (B + 1) / 2);
    double *vals = reinterpret_cast<double *>(staging.p);
    auto *status = reinterpret_cast<std::uint32_t *>(vals + host.size());
    // `host` is temporary: the stream is synchronised once before it goes -- right after the upload
    // (ahead of the encode) when no status is read, else with the status download at the end; the
    // guard covers a throw in between
    struct SyncAtExit
    {
        mhe_ctx *eng;
        void *s;
        bool armed = false;
        ~SyncAtExit()
        {
            if (armed) (void)mhe_stream_sync(eng, s);
        }
    } pending{ eng, s };
    if (!host.empty())
    {
        chk(mhe_memcpy_h2d(eng, vals, host.data(), host.size() * sizeof(double), s));
        pending.armed = true;
        if (!checked)
        {
            pending.armed = false;
            chk(mhe_stream_sync(eng, s));
        }
    }
    // fresh plaintexts: the destinations change only when every entry has been accepted
    std::vector<Plaintext> fresh(B);
    std::vector<const double *> in(B);
    std::vector<std::uint64_t *> out(B);
    for (std::size_t b = 0; b < B; b++)
    {
        fresh[b].set_level(ctx_, parms_id, L);
        fresh[b].scale() = scale;
        in[b] = vals + b * per;
        out[b] = fresh[b].store().dev_write(s, true);
    }
    chk(mhe_ckks_encode_dev(eng, enc_, (int)B, in.data(), count, is_complex ? 1 : 0, scale, (int)L, (int)L, out.data(),
                            l1.data(), status, s));
    if (checked)
    {
        std::vector<std::uint32_t> st(B);
        chk(mhe_memcpy_d2h(eng, st.data(), status, B * sizeof(std::uint32_t), s));
        pending.armed = false;
        chk(mhe_stream_sync(eng, s));
        for (std::uint32_t w : st)
            if (w) throw std::invalid_argument("encoded values are too large");
    }
    for (std::size_t b = 0; b < B; b++) *destinations[b] = std::move(fresh[b]);
}

// encode_many one entry at a time (batched launches off, or a trace that keeps one record per
// entry), also into fresh plaintexts: a throwing entry leaves every destination as it was
template <class V>
static void encode_each(CKKSEncoder &encoder, const std::vector<const V *> &values, parms_id_type parms_id,
                        double scale, const std::vector<Plaintext *> &destinations)
{
    std::vector<Plaintext> fresh(values.size());
    for (std::size_t i = 0; i < values.size(); i++) encoder.encode(*values[i], parms_id, scale, fresh[i]);
    for (std::size_t i = 0; i < values.size(); i++) *destinations[i] = std::move(fresh[i]);
}

template <class V>
static std::size_t check_many(const std::vector<const V *> &values, const std::vector<Plaintext *> &destinations)
{
    if (values.size() != destinations.size())
        throw std::invalid_argument("values and destinations differ in number");
    for (std::size_t i = 0; i < values.size(); i++)
    {
        if (!values[i] || !destinations[i]) throw std::invalid_argument("values and destinations cannot be null");
        if (values[i]->size() != values[0]->size()) throw std::invalid_argument("values must have one size");
        for (std::size_t j = 0; j < i; j++)
            if (destinations[j] == destinations[i]) throw std::invalid_argument("destinations must be distinct");
    }
    return values.empty() ? 0 : values[0]->size();
}

void CKKSEncoder::encode_many(const std::vector<const std::vector<double> *> &values, parms_id_type parms_id,
                              double scale, const std::vector<Plaintext *> &destinations)
{
    const std::size_t count = check_many(values, destinations);
    if (!batched_launches() || trace::enabled())
    {
        encode_each(*this, values, parms_id, scale, destinations);
        return;
    }
    if (values.empty()) return;
    std::vector<const double *> data(values.size());
    for (std::size_t i = 0; i < values.size(); i++) data[i] = values[i]->data();
    encode_many_internal(data, count, false, parms_id, scale, destinations);
}

void CKKSEncoder::encode_many(const std::vector<const std::vector<std::complex<double>> *> &values,
                              parms_id_type parms_id, double scale, const std::vector<Plaintext *> &destinations)
{
    const std::size_t count = check_many(values, destinations);
    if (!batched_launches() || trace::enabled())
    {
        encode_each(*this, values, parms_id, scale, destinations);
        return;
    }
    if (values.empty()) return;
    // complex<double> is laid out as (re, im): the interleaved pairs the engine reads
    std::vector<const double *> data(values.size());
    for (std::size_t i = 0; i < values.size(); i++) data[i] = reinterpret_cast<const double *>(values[i]->data());
    encode_many_internal(data, count, true, parms_id, scale, destinations);
}

void CKKSEncoder::encode(const std::vector<double> &values, double scale, Plaintext &destination, MemoryPoolHandle)
{
    encode(values, ctx_.first_parms_id(), scale, destination);
}

void CKKSEncoder::encode(const std::vector<std::complex<double>> &values, double scale, Plaintext &destination,
                         MemoryPoolHandle)
{
    encode(values, ctx_.first_parms_id(), scale, destination);
}

void CKKSEncoder::encode(double value, parms_id_type parms_id, double scale, Plaintext &destination, MemoryPoolHandle)
{
    TRACE_OP("encode_const", trace::pt(destination));
    TRACE_EXTRA("\"value\": " + trace::num(value) + ", \"scale\": " + trace::num(scale) + ", \"limbs\": " +
                std::to_string(ctx_.get_context_data(parms_id) ? ctx_.get_context_data(parms_id)->parms().coeff_modulus().size() : 0));
    auto cd = ctx_.get_context_data(parms_id);
    if (!cd) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    const std::size_t L = cd->parms().coeff_modulus().size();
    std::vector<std::uint64_t> r(L);
    chk(mhe_ckks_encode_scalar(ctx_.engine(), value, scale, (int)L, r.data()));
    void *s = ctx_.stream();
    destination.set_level(ctx_, parms_id, L);
    destination.scale() = scale;
    chk(mhe_set_scalar(ctx_.engine(), r.data(), destination.store().dev_write(s, true), 1, (int)L, s));
}

void CKKSEncoder::encode(double value, double scale, Plaintext &destination, MemoryPoolHandle)
{
    encode(value, ctx_.first_parms_id(), scale, destination);
}

void CKKSEncoder::decode_internal(const Plaintext &plain, std::vector<std::complex<double>> &out)
{
    if (!plain.is_ntt_form()) throw std::invalid_argument("plain is not in NTT form");
    auto cd = ctx_.get_context_data(plain.parms_id());
    if (!cd) throw std::invalid_argument("plain is not valid for encryption parameters");
    const std::size_t L = cd->parms().coeff_modulus().size();
    mhe_ctx *eng = ctx_.engine();
    void *s = ctx_.stream();
    // the slots are decoded on the device as interleaved (re, im) doubles -- complex<double>'s
    // layout -- and downloaded straight into the destination
    DevBuf z(eng, s, 2 * sparse_slots_);
    chk(mhe_ckks_decode_dev(eng, enc_, plain.store().dev_read(s), (int)L, plain.scale(),
                            sparse_slots_ == slots_ ? 0 : sparse_slots_, reinterpret_cast<double *>(z.p), s));
    out.resize(sparse_slots_);
    chk(mhe_memcpy_d2h(eng, out.data(), z.p, sparse_slots_ * sizeof(std::complex<double>), s));
    chk(mhe_stream_sync(eng, s));
}

void CKKSEncoder::decode(const Plaintext &plain, std::vector<std::complex<double>> &destination, MemoryPoolHandle)
{
    decode_internal(plain, destination);
}

void CKKSEncoder::decode(const Plaintext &plain, std::vector<double> &destination, MemoryPoolHandle)
{
    std::vector<std::complex<double>> z;
    decode_internal(plain, z);
    destination.resize(z.size());
    for (std::size_t i = 0; i < z.size(); i++) destination[i] = z[i].real();
}

// ------------------------------------------------------------------------------ Encryptor
Encryptor::Encryptor(const SEALContext &context, const PublicKey &public_key)
    : ctx_(context), pk_(public_key), asymmetric_(true)
{
    require_set(context);
    if (public_key.parms_id() != context.key_parms_id())
        throw std::invalid_argument("public key is not valid for encryption parameters");
    rng_ = factory_of(context);
}

Encryptor::Encryptor(const SEALContext &context, const SecretKey &secret_key)
    : ctx_(context), sk_(secret_key), asymmetric_(false), has_sk_(true)
{
    require_set(context);
    if (secret_key.parms_id() != context.key_parms_id())
        throw std::invalid_argument("secret key is not valid for encryption parameters");
    rng_ = factory_of(context);
}

Encryptor::Encryptor(const SEALContext &context, const PublicKey &public_key, const SecretKey &secret_key)
    : Encryptor(context, public_key)
{
    set_secret_key(secret_key);
}

void Encryptor::set_public_key(const PublicKey &public_key)
{
    if (public_key.parms_id() != ctx_.key_parms_id())
        throw std::invalid_argument("public key is not valid for encryption parameters");
    pk_ = public_key;
    asymmetric_ = true;
}

void Encryptor::set_secret_key(const SecretKey &secret_key)
{
    if (secret_key.parms_id() != ctx_.key_parms_id())
        throw std::invalid_argument("secret key is not valid for encryption parameters");
    sk_ = secret_key;
    has_sk_ = true;
}

void Encryptor::encrypt_zero_at(std::size_t L, Ciphertext &dest, bool symmetric, prng_seed_type *public_seed) const
{
    // encryptor.cpp:88-166 (encrypt_zero_internal): public-key encryption runs one level up
    // (the key level for the first data level) and is divided and rounded down by the dropped
    // prime; secret-key encryption runs at the level itself.
    const std::size_t K = ctx_.key_size(), n = ctx_.key_context_data()->parms().poly_modulus_degree();
    mhe_ctx *eng = ctx_.engine();
    void *s = ctx_.stream();
    std::uint64_t *d = dest.store().dev_write(s, true);
    const prng_seed_type seed = rng_->next_seed();
    if (symmetric)
    {
        if (!has_sk_) throw std::logic_error("secret key is not set");
        sym_encrypt_zero(ctx_, seed, sk_.data().store().dev_read(s), L, d, d + L * n, s);
        if (public_seed) *public_seed = rnd::stream_prefix_seed(seed);
        return;
    }
    if (!asymmetric_) throw std::logic_error("public key is not set");
    // encrypt_zero_asymmetric (rlwe.cpp:220-286): one PRNG; u ternary, then e_0, e_1 (CBD)
    const std::size_t m = L < K ? L + 1 : L;
    const std::uint64_t *pk = pk_.data().store().dev_read(s);
    DevBuf u(eng, s, m * n), c(eng, s, 2 * m * n), e(eng, s, 2 * m * n), state(eng, s, 1);
    auto *st = reinterpret_cast<std::uint32_t *>(state.p);
    chk(mhe_prng_small(eng, seed.data(), 0, MHE_SAMPLE_TERNARY, (int)m, u.p, st, s));
    chk(mhe_prng_small(eng, seed.data(), 4 * n, MHE_SAMPLE_CBD, (int)m, e.p, st, s));
    chk(mhe_prng_small(eng, seed.data(), 10 * n, MHE_SAMPLE_CBD, (int)m, e.p + m * n, st, s));
    chk(mhe_ntt_forward(eng, u.p, 1, (int)m, 0, s));
    chk(mhe_ntt_forward(eng, e.p, 2, (int)m, 0, s));
    for (int j = 0; j < 2; j++)
    {
        // pk_j restricted to the first m primes: limbs 0..m-1 of poly j ([2][K][n] layout)
        chk(mhe_multiply_plain(eng, u.p, pk + j * K * n, c.p + j * m * n, 1, (int)m, s));
        chk(mhe_add(eng, e.p + j * m * n, c.p + j * m * n, c.p + j * m * n, 1, (int)m, s));
    }
    if (m == L)
        chk(mhe_memcpy_d2d(eng, d, c.p, 2 * L * n * 8, s));
    else
        chk(mhe_rescale_to_next(eng, c.p, d, 2, (int)m, s));
}

void Encryptor::zero_at(parms_id_type parms_id, Ciphertext &destination, bool symmetric,
                        prng_seed_type *public_seed) const
{
    auto cd = ctx_.get_context_data(parms_id);
    if (!cd) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    destination.resize(ctx_, parms_id, 2);
    destination.is_ntt_form() = true;
    destination.scale() = 1.0;
    encrypt_zero_at(cd->parms().coeff_modulus().size(), destination, symmetric, public_seed);
}

void Encryptor::encrypt_zero(parms_id_type parms_id, Ciphertext &destination, MemoryPoolHandle) const
{
    // SEAL's encrypt_zero / encrypt are public-key encryptions (encryptor.h:158-164, encryptor.cpp:
    // 177-181): without a public key they throw, even when a secret key is set
    zero_at(parms_id, destination, false, nullptr);
}

void Encryptor::encrypt_zero(Ciphertext &destination, MemoryPoolHandle pool) const
{
    encrypt_zero(ctx_.first_parms_id(), destination, pool);
}

void Encryptor::encrypt_zero_symmetric(parms_id_type parms_id, Ciphertext &destination, MemoryPoolHandle) const
{
    zero_at(parms_id, destination, true, nullptr);
}

void Encryptor::encrypt_zero_symmetric(Ciphertext &destination, MemoryPoolHandle pool) const
{
    encrypt_zero_symmetric(ctx_.first_parms_id(), destination, pool);
}

Serializable<Ciphertext> Encryptor::encrypt_zero_symmetric(parms_id_type parms_id, MemoryPoolHandle) const
{
    Ciphertext c;
    prng_seed_type seed{};
    zero_at(parms_id, c, true, &seed);
    return Serializable<Ciphertext>(std::move(c), SeedMap{ { 0, { seed } } });
}

Serializable<Ciphertext> Encryptor::encrypt_zero_symmetric(MemoryPoolHandle pool) const
{
    return encrypt_zero_symmetric(ctx_.first_parms_id(), pool);
}

void Encryptor::encrypt(const Plaintext &plain, Ciphertext &destination, MemoryPoolHandle) const
{
    encrypt_plain(plain, destination, false, nullptr);
}

Serializable<Ciphertext> Encryptor::encrypt(const Plaintext &plain, MemoryPoolHandle) const
{
    // a public-key encryption has no seed to save (encrypt_symmetric is the seeded form)
    Ciphertext c;
    encrypt_plain(plain, c, false, nullptr);
    return Serializable<Ciphertext>(std::move(c), SeedMap{});
}

void Encryptor::encrypt_symmetric(const Plaintext &plain, Ciphertext &destination, MemoryPoolHandle) const
{
    encrypt_plain(plain, destination, true, nullptr);
}

Serializable<Ciphertext> Encryptor::encrypt_symmetric(const Plaintext &plain, MemoryPoolHandle) const
{
    Ciphertext c;
    prng_seed_type seed{};
    encrypt_plain(plain, c, true, &seed);
    return Serializable<Ciphertext>(std::move(c), SeedMap{ { 0, { seed } } });
}

void Encryptor::encrypt_plain(const Plaintext &plain, Ciphertext &destination, bool symmetric,
                              prng_seed_type *public_seed) const
{
    TRACE_OP("encrypt", trace::ct(destination), trace::pt(plain));
    // encrypt_internal (encryptor.cpp:168-239), CKKS branch: the plaintext is added to c0 only, so a
    // symmetric encryption keeps c1 = the seeded uniform polynomial
    if (!plain.is_ntt_form()) throw std::invalid_argument("plain must be in NTT form");
    auto cd = ctx_.get_context_data(plain.parms_id());
    if (!cd) throw std::invalid_argument("plain is not valid for encryption parameters");
    const std::size_t L = cd->parms().coeff_modulus().size();
    zero_at(plain.parms_id(), destination, symmetric, public_seed);
    void *s = ctx_.stream();
    std::uint64_t *d = destination.store().dev_write(s);
    chk(mhe_add(ctx_.engine(), d, plain.store().dev_read(s), d, 1, (int)L, s));
    destination.scale() = plain.scale();
}

// The batch behind encrypt_many (plains given) and encrypt_zero_many (plains null), all at parms_id.
void Encryptor::encrypt_batch(parms_id_type parms_id, const std::vector<const Plaintext *> *plains,
                              const std::vector<Ciphertext *> &destinations) const
{
    const std::size_t B = destinations.size();
    if (plains && plains->size() != B) throw std::invalid_argument("plains and destinations differ in number");
    for (std::size_t i = 0; i < B; i++)
    {
        if (!destinations[i] || (plains && !(*plains)[i]))
            throw std::invalid_argument("plains and destinations cannot be null");
        for (std::size_t j = 0; j < i; j++)
            if (destinations[j] == destinations[i]) throw std::invalid_argument("destinations must be distinct");
    }
    for (std::size_t i = 0; plains && i < B; i++)
    {
        const Plaintext &plain = *(*plains)[i];
        if (!plain.is_ntt_form()) throw std::invalid_argument("plain must be in NTT form");
        if (!ctx_.get_context_data(plain.parms_id()))
            throw std::invalid_argument("plain is not valid for encryption parameters");
        if (plain.parms_id() != parms_id) throw std::invalid_argument("plains must be at one level");
    }
    auto cd = ctx_.get_context_data(parms_id);
    if (!cd) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    if (!asymmetric_) throw std::logic_error("public key is not set");
    if (!B) return;
    // fresh ciphertexts: the destinations change only when every entry has been issued
    std::vector<Ciphertext> fresh(B);
    if (!batched_launches() || trace::enabled())
    {
        // entry by entry (a trace keeps one record per entry), as encode_each does
        for (std::size_t i = 0; i < B; i++)
        {
            if (plains)
                encrypt(*(*plains)[i], fresh[i]);
            else
                encrypt_zero(parms_id, fresh[i]);
        }
    }
    else
    {
        const std::size_t L = cd->parms().coeff_modulus().size(), K = ctx_.key_size();
        void *s = ctx_.stream();
        std::vector<prng_seed_type> seeds(B);
        std::vector<const std::uint64_t *> in(B, nullptr);
        std::vector<std::uint64_t *> out(B);
        static_assert(sizeof(prng_seed_type) == 8 * sizeof(std::uint64_t), "a seed is eight words");
        for (std::size_t i = 0; i < B; i++)
        {
            seeds[i] = rng_->next_seed(); // one per entry, in order: the seeds of the single calls
            fresh[i].resize(ctx_, parms_id, 2);
            fresh[i].is_ntt_form() = true;
            fresh[i].scale() = plains ? (*plains)[i]->scale() : 1.0;
            out[i] = fresh[i].store().dev_write(s, true);
            if (plains) in[i] = (*plains)[i]->store().dev_read(s);
        }
        chk(mhe_encrypt_pk_batch(ctx_.engine(), (int)B, reinterpret_cast<const std::uint64_t(*)[8]>(seeds.data()),
                                 pk_.data().store().dev_read(s), (int)K, plains ? in.data() : nullptr, out.data(), (int)L,
                                 s));
    }
    for (std::size_t i = 0; i < B; i++) *destinations[i] = std::move(fresh[i]);
}

void Encryptor::encrypt_many(const std::vector<const Plaintext *> &plains,
                             const std::vector<Ciphertext *> &destinations) const
{
    parms_id_type id = ctx_.first_parms_id();
    for (const Plaintext *p : plains)
        if (p)
        {
            id = p->parms_id();
            break;
        }
    encrypt_batch(id, &plains, destinations);
}

void Encryptor::encrypt_zero_many(parms_id_type parms_id, const std::vector<Ciphertext *> &destinations) const
{
    encrypt_batch(parms_id, nullptr, destinations);
}

// ------------------------------------------------------------------------------ Decryptor
Decryptor::Decryptor(const SEALContext &context, const SecretKey &secret_key) : ctx_(context), sk_(secret_key)
{
    require_set(context);
    if (secret_key.parms_id() != context.key_parms_id())
        throw std::invalid_argument("secret key is not valid for encryption parameters");
}

void Decryptor::decrypt(const Ciphertext &encrypted, Plaintext &destination)
{
    // decryptor.cpp ckks_decrypt: <(c0, c1, c2, ...), (1, s, s^2, ...)> in NTT form
    auto cd = ctx_.get_context_data(encrypted.parms_id());
    if (!cd || encrypted.size() < 2) throw std::invalid_argument("encrypted is not valid for encryption parameters");
    if (!encrypted.is_ntt_form()) throw std::invalid_argument("encrypted must be in NTT form");
    const std::size_t L = cd->parms().coeff_modulus().size();
    mhe_ctx *eng = ctx_.engine();
    void *s = ctx_.stream();
    const std::uint64_t *c = encrypted.store().dev_read(s);
    const std::uint64_t *sk = sk_.data().store().dev_read(s);
    Plaintext out;
    out.set_level(ctx_, encrypted.parms_id(), L);
    std::uint64_t *d = out.store().dev_write(s, true);
    chk(mhe_decrypt(eng, c, (int)encrypted.size(), sk, d, (int)L, s));
    out.scale() = encrypted.scale();
    destination = std::move(out);
}
} // namespace seal
