// evaluator.cpp -- the single-call Evaluator entry points: each is one or a few libmhe calls on the
// calling thread's stream plus the bookkeeping SEAL keeps around them (parms_id chain, scales, sizes,
// argument checks and their messages).  One body per operation: its preconditions are a named
// function and where its result goes is a Placed (seal_internal.h).  Line numbers cite evaluator.cpp
// of the modified SEAL 3.6.6 (gpt2_ckks/gpt2-ckks/single-key/seal-modified-3.6.6/native/src/seal/).
#include "seal_internal.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

namespace seal
{
// ------------------------------------------------------------------------------ argument checks
Level level_of(const SEALContext &ctx, const parms_id_type &id, const char *what)
{
    auto cd = ctx.get_context_data(id);
    if (!cd) throw std::invalid_argument(std::string(what) + " is not valid for encryption parameters");
    return { cd->parms().coeff_modulus().size(), cd->parms().poly_modulus_degree(),
             (double)cd->total_coeff_modulus_bit_count(), cd };
}

Level check_ct(const SEALContext &ctx, const Ciphertext &ct, const char *what)
{
    Level lv = level_of(ctx, ct.parms_id(), what);
    if (ct.size() < 2 || ct.coeff_modulus_size() != lv.L || ct.store().words() != ct.size() * lv.L * lv.n ||
        ct.store().engine() != ctx.engine())
        throw std::invalid_argument(std::string(what) + " is not valid for encryption parameters");
    return lv;
}

void check_scale(double scale, const Level &lv)
{
    if (scale <= 0 || static_cast<int>(std::log2(scale)) >= (int)lv.total_bits)
        throw std::invalid_argument("scale out of bounds (2^" + std::to_string(std::log2(scale)) + " at " +
                                    std::to_string(lv.L) + " limbs, " + std::to_string(lv.total_bits) + " bits)");
}

void check_pair(const SEALContext &ctx, const Ciphertext &a, const Ciphertext &b, bool scales)
{
    check_ct(ctx, a, "encrypted1");
    check_ct(ctx, b, "encrypted2");
    if (a.parms_id() != b.parms_id()) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
    if (a.is_ntt_form() != b.is_ntt_form()) throw std::invalid_argument("NTT form mismatch");
    if (scales && !are_close(a.scale(), b.scale())) throw std::invalid_argument("scale mismatch");
}

void check_key_parms(const SEALContext &ctx, const KSwitchKeys &keys, const char *what)
{
    if (keys.parms_id() != ctx.key_parms_id())
        throw std::invalid_argument(std::string(what) + " is not valid for encryption parameters");
}

Level check_product(const SEALContext &ctx, const Ciphertext &a, const Ciphertext &b, double &new_scale)
{
    check_ct(ctx, a, "encrypted1");
    check_ct(ctx, b, "encrypted2");
    if (a.parms_id() != b.parms_id()) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
    if (!a.is_ntt_form() || !b.is_ntt_form())
        throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form");
    if (a.size() != 2 || b.size() != 2)
        throw std::logic_error("only size-2 ciphertexts are multiplied (relinearize first)");
    Level lv = level_of(ctx, a.parms_id(), "encrypted1");
    new_scale = a.scale() * b.scale();
    check_scale(new_scale, lv);
    return lv;
}

Level check_square(const SEALContext &ctx, const Ciphertext &ct, double &new_scale)
{
    Level lv = check_ct(ctx, ct, "encrypted");
    if (!ct.is_ntt_form()) throw std::invalid_argument("encrypted must be in NTT form");
    if (ct.size() != 2) throw std::logic_error("only size-2 ciphertexts are squared (relinearize first)");
    new_scale = ct.scale() * ct.scale();
    check_scale(new_scale, lv);
    return lv;
}

const char *galois_fault(const SEALContext &ctx, const Ciphertext &ct, std::size_t n, std::uint32_t elt,
                         const GaloisKeys &keys)
{
    if (keys.parms_id() != ctx.key_parms_id()) return "galois_keys is not valid for encryption parameters";
    if (!(elt & 1) || elt >= 2 * n) return "Galois element is not valid";
    if (ct.size() > 2) return "encrypted size must be 2";
    if (!ct.is_ntt_form()) return "encrypted must be in NTT form";
    if (!keys.has_key(elt)) return "Galois key not present";
    return nullptr;
}

Level check_galois(const SEALContext &ctx, const Ciphertext &ct, std::uint32_t elt, const GaloisKeys &keys)
{
    Level lv = check_ct(ctx, ct, "encrypted");
    if (const char *fault = galois_fault(ctx, ct, lv.n, elt, keys)) throw std::invalid_argument(fault);
    return lv;
}

Rescale check_rescale(const SEALContext &ctx, const Ciphertext &ct)
{
    Level lv = check_ct(ctx, ct, "encrypted");
    if (ctx.last_parms_id() == ct.parms_id()) throw std::invalid_argument("end of modulus switching chain reached");
    if (!ct.is_ntt_form()) throw std::invalid_argument("CKKS encrypted must be in NTT form");
    auto next = lv.cd->next_context_data();
    const double q_last = (double)lv.cd->parms().coeff_modulus().back().value();
    const double new_scale = ct.scale() / q_last;
    check_scale(new_scale, level_of(ctx, next->parms_id(), "parms_id"));
    return { lv, next->parms_id(), new_scale };
}

// add_const / multiply_const (evaluator.cpp:287-310) encode the constant at the first level and
// mod-switch it to the ciphertext's level; the engine produces exactly those residues
std::vector<std::uint64_t> scalar_residues(const SEALContext &ctx, const Ciphertext &ct, double value, Level &lv)
{
    lv = check_ct(ctx, ct, "encrypted");
    const std::size_t L1 = ctx.first_context_data()->parms().coeff_modulus().size();
    std::vector<std::uint64_t> r(lv.L);
    chk(mhe_ckks_encode_scalar_at(ctx.engine(), value, ct.scale(), (int)L1, (int)lv.L, r.data()));
    if (!ct.is_ntt_form()) throw std::invalid_argument("NTT form mismatch");
    return r;
}

StepKey step_key(std::size_t n, int step, const GaloisKeys &keys)
{
    const std::uint32_t elt = mhe_galois_elt_from_step(__builtin_ctzll(n), step);
    if (!elt) throw std::invalid_argument("step count too large");
    return { elt, keys.has_key(elt) };
}

// ------------------------------------------------------------------------------ result placement
void fresh_dest(const SEALContext &ctx, const Ciphertext &src, Ciphertext &dst, std::size_t size)
{
    dst.resize(ctx, src.parms_id(), 0);
    dst.resize(size);
    dst.scale() = src.scale();
    dst.is_ntt_form() = src.is_ntt_form();
}

Placed::Placed(const SEALContext &ctx, How how, const Ciphertext &src, Ciphertext &dst, std::size_t size,
               std::size_t limbs)
    : ctx_(ctx), how_(how), src_(src), dst_(dst), size_(size), ntt_(src.is_ntt_form())
{
    if (how_ == fresh)
    {
        store_.bind(ctx);
        store_.resize_words(size * limbs * src.poly_modulus_degree(), false);
    }
    else if (how_ == reuse)
        fresh_dest(ctx, src, dst, size);
}

std::uint64_t *Placed::out(void *s)
{
    if (!out_) out_ = how_ == fresh ? store_.dev_write(s, true) : dst_.store().dev_write(s, how_ == reuse);
    return out_;
}

const std::uint64_t *Placed::in(void *s) { return how_ == same ? out(s) : src_.store().dev_read(s); }

void Placed::commit(const parms_id_type &id, double scale)
{
    if (how_ == fresh)
    {
        dst_.store() = std::move(store_);
        dst_.resize(ctx_, id, size_);
        dst_.is_ntt_form() = ntt_;
    }
    dst_.scale() = scale;
}

void mulre_product(const SEALContext &ctx, const Ciphertext &a, const Ciphertext &b, Ciphertext &destination)
{
    check_pair(ctx, a, b, false);
    const Level lv = level_of(ctx, a.parms_id(), "encrypted1");
    void *s = ctx.stream();
    const std::uint64_t *pa = a.store().dev_read(s), *pb = b.store().dev_read(s);
    const double new_scale = b.scale() * b.scale();
    check_scale(new_scale, lv);
    Placed out(ctx, Placed::reuse, a, destination, 3, lv.L);
    chk(mhe_ct_multiply(ctx.engine(), pa, pb, out.out(s), (int)lv.L, s));
    out.commit(a.parms_id(), new_scale);
}

// ------------------------------------------------------------------------------ Evaluator
struct Evaluator::VecCache
{
    struct Key
    {
        std::uint64_t hi, lo;
        std::size_t limbs;
        std::uint64_t scale_bits;
        bool operator<(const Key &o) const
        {
            return std::tie(hi, lo, limbs, scale_bits) < std::tie(o.hi, o.lo, o.limbs, o.scale_bits);
        }
    };
    std::mutex mu;
    std::map<Key, Plaintext> entries;
    std::size_t bytes = 0;
    std::size_t cap = [] {
        const char *e = std::getenv("MHE_VEC_CACHE_GB");
        const double gb = e ? std::atof(e) : 48.0;
        return gb > 0 ? (std::size_t)(gb * 1e9) : (std::size_t)0;
    }();
};

Evaluator::Evaluator(const SEALContext &context, CKKSEncoder &encoder)
    : context_(context), encoder_(encoder), vcache_(std::make_shared<VecCache>())
{
    if (!context.parameters_set()) throw std::invalid_argument("encryption parameters are not set correctly");
}

const Plaintext &Evaluator::cached_vector_plain(const Ciphertext &encrypted, std::uint64_t id_hi, std::uint64_t id_lo,
                                                const std::function<std::vector<double>()> &make,
                                                Plaintext &scratch) const
{
    const Level lv = check_ct(context_, encrypted, "encrypted");
    std::uint64_t sb;
    const double sc = encrypted.scale();
    std::memcpy(&sb, &sc, sizeof sb);
    const VecCache::Key key{ id_hi, id_lo, lv.L, sb };
    VecCache &vc = *vcache_;
    const std::size_t sz = lv.L * lv.n * sizeof(std::uint64_t);
    bool fits;
    {
        std::lock_guard<std::mutex> g(vc.mu);
        auto it = vc.entries.find(key);
        if (it != vc.entries.end()) return it->second;
        fits = vc.cap > 0 && vc.bytes + sz <= vc.cap;
    }
    if (!fits)
    {
        encode_vector_for(encrypted, make(), scratch);
        return scratch;
    }
    Plaintext pt;
    encode_vector_for(encrypted, make(), pt);
    std::lock_guard<std::mutex> g(vc.mu);
    auto r = vc.entries.emplace(key, std::move(pt)); // another thread may have made the same entry
    if (r.second) vc.bytes += sz;
    return r.first->second;
}

std::size_t Evaluator::vector_cache_entries() const
{
    std::lock_guard<std::mutex> g(vcache_->mu);
    return vcache_->entries.size();
}

std::size_t Evaluator::vector_cache_bytes() const
{
    std::lock_guard<std::mutex> g(vcache_->mu);
    return vcache_->bytes;
}

void Evaluator::negate_inplace(Ciphertext &encrypted) const { negate(encrypted, encrypted); }

void Evaluator::negate(const Ciphertext &encrypted, Ciphertext &destination) const
{
    TRACE_OP("negate", trace::ct(destination), trace::ct(encrypted));
    // evaluator.cpp:78-101
    Level lv = check_ct(context_, encrypted, "encrypted");
    void *s = context_.stream();
    const std::size_t size = encrypted.size();
    Placed out = Placed::onto(context_, encrypted, destination, lv.L);
    const std::uint64_t *a = out.in(s);
    chk(mhe_negate(context_.engine(), a, out.out(s), (int)size, (int)lv.L, s));
}

// evaluator.cpp:103-164 (add), 187-246 (sub): the common components +-, the rest of a longer
// encrypted2 copied (add) or negated (sub)
static void add_sub(const SEALContext &ctx, Ciphertext &encrypted1, const Ciphertext &encrypted2, bool sub)
{
    check_pair(ctx, encrypted1, encrypted2, true);
    const std::size_t L = encrypted1.coeff_modulus_size(), n = encrypted1.poly_modulus_degree();
    const std::size_t s1 = encrypted1.size(), s2 = encrypted2.size(), mn = std::min(s1, s2), rest = mn * L * n;
    void *s = ctx.stream();
    if (s1 < s2) encrypted1.resize(ctx, encrypted1.parms_id(), s2);
    const std::uint64_t *b = encrypted2.store().dev_read(s);
    std::uint64_t *a = encrypted1.store().dev_write(s);
    chk((sub ? mhe_sub : mhe_add)(ctx.engine(), a, b, a, (int)mn, (int)L, s));
    if (s1 < s2 && sub)
        chk(mhe_negate(ctx.engine(), b + rest, a + rest, (int)(s2 - mn), (int)L, s));
    else if (s1 < s2)
        chk(mhe_memcpy_d2d(ctx.engine(), a + rest, b + rest, (s2 - mn) * L * n * 8, s));
}

void Evaluator::add_inplace(Ciphertext &encrypted1, const Ciphertext &encrypted2) const
{
    TRACE_OP("add", trace::ct(encrypted1), trace::ct(encrypted1), trace::ct(encrypted2));
    add_sub(context_, encrypted1, encrypted2, false);
}

void Evaluator::add(const Ciphertext &encrypted1, const Ciphertext &encrypted2, Ciphertext &destination) const
{
    TRACE_OP("add", trace::ct(destination), trace::ct(encrypted1), trace::ct(encrypted2));
    if (&encrypted2 == &destination)
        add_inplace(destination, encrypted1);
    else if (&encrypted1 != &destination && encrypted1.size() == encrypted2.size())
    {
        // SEAL copies encrypted1 then adds; writing the sum directly saves a pass over HBM
        check_pair(context_, encrypted1, encrypted2, true);
        void *s = context_.stream();
        destination.resize(context_, encrypted1.parms_id(), encrypted1.size());
        const std::uint64_t *a = encrypted1.store().dev_read(s), *b = encrypted2.store().dev_read(s);
        chk(mhe_add(context_.engine(), a, b, destination.store().dev_write(s, true), (int)encrypted1.size(),
                    (int)encrypted1.coeff_modulus_size(), s));
        destination.scale() = encrypted1.scale();
        destination.is_ntt_form() = encrypted1.is_ntt_form();
    }
    else
    {
        destination = encrypted1;
        add_inplace(destination, encrypted2);
    }
}

void Evaluator::add_many(const std::vector<Ciphertext> &encrypteds, Ciphertext &destination) const
{
    // evaluator.cpp:166-185
    if (encrypteds.empty()) throw std::invalid_argument("encrypteds cannot be empty");
    for (auto &e : encrypteds)
        if (&e == &destination) throw std::invalid_argument("encrypteds must be different from destination");
    destination = encrypteds[0];
    for (std::size_t i = 1; i < encrypteds.size(); i++) add_inplace(destination, encrypteds[i]);
}

void Evaluator::sub_inplace(Ciphertext &encrypted1, const Ciphertext &encrypted2) const
{
    TRACE_OP("sub", trace::ct(encrypted1), trace::ct(encrypted1), trace::ct(encrypted2));
    add_sub(context_, encrypted1, encrypted2, true);
}

void Evaluator::sub(const Ciphertext &encrypted1, const Ciphertext &encrypted2, Ciphertext &destination) const
{
    TRACE_OP("sub", trace::ct(destination), trace::ct(encrypted1), trace::ct(encrypted2));
    if (&encrypted2 == &destination)
    {
        sub_inplace(destination, encrypted1);
        negate_inplace(destination);
    }
    else
    {
        destination = encrypted1;
        sub_inplace(destination, encrypted2);
    }
}

// ckks_multiply (evaluator.cpp:673-773, size 2 x size 2 -> 3): in place the product goes to a fresh
// store, out of place (destination not an input) into the destination's allocation
static void ct_product(const SEALContext &ctx, const Ciphertext &a, const Ciphertext &b, Ciphertext &destination,
                Placed::How how)
{
    double new_scale;
    Level lv = check_product(ctx, a, b, new_scale);
    void *s = ctx.stream();
    Placed out(ctx, how, a, destination, 3, lv.L);
    const std::uint64_t *pa = a.store().dev_read(s), *pb = b.store().dev_read(s);
    chk(mhe_ct_multiply(ctx.engine(), pa, pb, out.out(s), (int)lv.L, s));
    out.commit(a.parms_id(), new_scale);
}

void Evaluator::multiply_inplace(Ciphertext &encrypted1, const Ciphertext &encrypted2, MemoryPoolHandle) const
{
    TRACE_OP("multiply", trace::ct(encrypted1), trace::ct(encrypted1), trace::ct(encrypted2));
    // evaluator.cpp:248-285
    ct_product(context_, encrypted1, encrypted2, encrypted1, Placed::fresh);
}

void Evaluator::multiply(const Ciphertext &encrypted1, const Ciphertext &encrypted2, Ciphertext &destination,
                         MemoryPoolHandle) const
{
    TRACE_OP("multiply", trace::ct(destination), trace::ct(encrypted1), trace::ct(encrypted2));
    if (&encrypted1 != &destination && &encrypted2 != &destination && encrypted1.size() == 2 &&
        encrypted2.size() == 2)
        // ckks_multiply into a fresh destination (SEAL copies encrypted1 first)
        ct_product(context_, encrypted1, encrypted2, destination, Placed::reuse);
    else if (&encrypted2 == &destination)
        multiply_inplace(destination, encrypted1);
    else
    {
        destination = encrypted1;
        multiply_inplace(destination, encrypted2);
    }
}

void Evaluator::multiply_many(const std::vector<Ciphertext> &encrypteds, const RelinKeys &, Ciphertext &destination,
                              MemoryPoolHandle) const
{
    // evaluator.cpp:1468-1543: BFV only in SEAL 3.6
    if (encrypteds.empty()) throw std::invalid_argument("encrypteds vector must not be empty");
    for (auto &e : encrypteds)
        if (&e == &destination) throw std::invalid_argument("encrypteds must be different from destination");
    level_of(context_, encrypteds[0].parms_id(), "encrypteds");
    throw std::logic_error("unsupported scheme");
}

void Evaluator::exponentiate_inplace(Ciphertext &encrypted, std::uint64_t exponent, const RelinKeys &relin_keys,
                                     MemoryPoolHandle) const
{
    // evaluator.cpp:1545-1576 (delegates to multiply_many: BFV only)
    level_of(context_, encrypted.parms_id(), "encrypted");
    if (!context_.get_context_data(relin_keys.parms_id()))
        throw std::invalid_argument("relin_keys is not valid for encryption parameters");
    if (exponent == 0) throw std::invalid_argument("exponent cannot be 0");
    if (exponent == 1) return;
    throw std::logic_error("unsupported scheme");
}

void Evaluator::square_inplace(Ciphertext &encrypted, MemoryPoolHandle) const { square(encrypted, encrypted); }

void Evaluator::square(const Ciphertext &encrypted, Ciphertext &destination, MemoryPoolHandle) const
{
    TRACE_OP("square", trace::ct(destination), trace::ct(encrypted));
    // evaluator.cpp:816-845, ckks_square :1000-1059; in place the square goes to a fresh store
    double new_scale;
    Level lv = check_square(context_, encrypted, new_scale);
    void *s = context_.stream();
    Placed out(context_, &encrypted == &destination ? Placed::fresh : Placed::reuse, encrypted, destination, 3, lv.L);
    const std::uint64_t *a = encrypted.store().dev_read(s);
    chk(mhe_ct_square(context_.engine(), a, out.out(s), (int)lv.L, s));
    out.commit(encrypted.parms_id(), new_scale);
}

void Evaluator::switch_key(Ciphertext &encrypted, const std::uint64_t *target, const KSwitchKeys &keys,
                           std::size_t index) const
{
    // switch_key_inplace (evaluator.cpp:2281-2525): ct[0..1] += KS(target)
    const std::size_t L = encrypted.coeff_modulus_size();
    void *s = context_.stream();
    std::size_t kl = 0;
    const std::uint64_t *key = keys.key_for(index, L, s, kl);
    std::uint64_t *ct = encrypted.store().dev_write(s);
    chk(mhe_switch_key(context_.engine(), ct, target, key, (int)kl, (int)L, s));
}

void Evaluator::relinearize_inplace(Ciphertext &encrypted, const RelinKeys &relin_keys, MemoryPoolHandle) const
{
    if (merge_point([&] { return LsOp{ LsOp::RELIN, {}, {}, {}, { &encrypted }, nullptr, &relin_keys }; })) return;
    TRACE_OP("relinearize", trace::ct(encrypted), trace::ct(encrypted));
    // relinearize_internal (evaluator.cpp:1061-1116)
    Level lv = check_ct(context_, encrypted, "encrypted");
    check_key_parms(context_, relin_keys, "relin_keys");
    if (!encrypted.is_ntt_form()) throw std::invalid_argument("encrypted must be in NTT form");
    void *s = context_.stream();
    std::size_t size = encrypted.size();
    if (size == 3)
    {
        std::size_t kl = 0;
        const std::uint64_t *key = relin_keys.key_for(RelinKeys::get_index(2), lv.L, s, kl);
        std::uint64_t *ct = encrypted.store().dev_write(s);
        chk(mhe_relinearize(context_.engine(), ct, key, (int)kl, (int)lv.L, s));
        size = 2;
    }
    while (size > 2)
    {
        // fold the last component with the key for s^(size-1)
        std::uint64_t *ct = encrypted.store().dev_write(s);
        switch_key(encrypted, ct + (size - 1) * lv.L * lv.n, relin_keys, RelinKeys::get_index(size - 1));
        size--;
    }
    encrypted.resize(size);
}

void Evaluator::relinearize(const Ciphertext &encrypted, const RelinKeys &relin_keys, Ciphertext &destination,
                            MemoryPoolHandle) const
{
    TRACE_OP("relinearize", trace::ct(destination), trace::ct(encrypted));
    destination = encrypted;
    relinearize_inplace(destination, relin_keys);
}

void Evaluator::mod_switch_to_next_inplace(Ciphertext &encrypted, MemoryPoolHandle) const
{
    TRACE_OP("mod_switch", trace::ct(encrypted), trace::ct(encrypted));
    // mod_switch_drop_to_next (evaluator.cpp:1183-1246) -- CKKS mod_switch_to_next
    Level lv = check_ct(context_, encrypted, "encrypted");
    if (!encrypted.is_ntt_form()) throw std::invalid_argument("CKKS encrypted must be in NTT form");
    auto next = lv.cd->next_context_data();
    if (!next) throw std::invalid_argument("end of modulus switching chain reached");
    void *s = context_.stream();
    const std::size_t size = encrypted.size();
    Placed out(context_, Placed::fresh, encrypted, encrypted, size, lv.L - 1);
    const std::uint64_t *p = encrypted.store().dev_read(s);
    chk(mhe_mod_switch_drop(context_.engine(), p, out.out(s), (int)size, (int)lv.L, s));
    out.commit(next->parms_id(), encrypted.scale());
}

void Evaluator::mod_switch_to_next(const Ciphertext &encrypted, Ciphertext &destination, MemoryPoolHandle) const
{
    TRACE_OP("mod_switch", trace::ct(destination), trace::ct(encrypted));
    destination = encrypted;
    mod_switch_to_next_inplace(destination);
}

void Evaluator::mod_switch_to_next_inplace(Plaintext &plain) const
{
    TRACE_OP("pt_mod_switch", trace::pt(plain), trace::pt(plain));
    // mod_switch_drop_to_next(Plaintext) (evaluator.cpp:1248-1281)
    if (!plain.is_ntt_form()) throw std::invalid_argument("plain is not in NTT form");
    Level lv = level_of(context_, plain.parms_id(), "plain");
    auto next = lv.cd->next_context_data();
    if (!next) throw std::invalid_argument("end of modulus switching chain reached");
    const double scale = plain.scale();
    plain.set_level(context_, next->parms_id(), lv.L - 1); // shrinking keeps the first L-1 limbs
    plain.scale() = scale;
}

// evaluator.cpp:1326-1340, 1416-1430: the ciphertext's level and the level to go down to
static Level check_target(const SEALContext &ctx, const Ciphertext &encrypted, const parms_id_type &parms_id, Level &target)
{
    Level cur = check_ct(ctx, encrypted, "encrypted");
    target = level_of(ctx, parms_id, "parms_id");
    if (cur.cd->chain_index() < target.cd->chain_index())
        throw std::invalid_argument("cannot switch to higher level modulus");
    return cur;
}

void Evaluator::mod_switch_to_inplace(Ciphertext &encrypted, parms_id_type parms_id, MemoryPoolHandle) const
{
    TRACE_OP("mod_switch", trace::ct(encrypted), trace::ct(encrypted));
    // evaluator.cpp:1326-1348
    Level target, cur = check_target(context_, encrypted, parms_id, target);
    if (encrypted.parms_id() == parms_id) return;
    if (!encrypted.is_ntt_form()) throw std::invalid_argument("CKKS encrypted must be in NTT form");
    // all dropped limbs at once: copy the kept prefix of every component
    const std::size_t L2 = target.L, n = cur.n, size = encrypted.size();
    void *s = context_.stream();
    Placed out(context_, Placed::fresh, encrypted, encrypted, size, L2);
    std::uint64_t *d = out.out(s);
    const std::uint64_t *p = encrypted.store().dev_read(s);
    for (std::size_t k = 0; k < size; k++)
        chk(mhe_memcpy_d2d(context_.engine(), d + k * L2 * n, p + k * cur.L * n, L2 * n * 8, s));
    out.commit(parms_id, encrypted.scale());
}

void Evaluator::mod_switch_to(const Ciphertext &encrypted, parms_id_type parms_id, Ciphertext &destination,
                              MemoryPoolHandle) const
{
    TRACE_OP("mod_switch", trace::ct(destination), trace::ct(encrypted));
    destination = encrypted;
    mod_switch_to_inplace(destination, parms_id);
}

void Evaluator::mod_switch_to_inplace(Plaintext &plain, parms_id_type parms_id) const
{
    TRACE_OP("pt_mod_switch", trace::pt(plain), trace::pt(plain));
    // evaluator.cpp:1350-1376
    auto cur = context_.get_context_data(plain.parms_id());
    auto target = context_.get_context_data(parms_id);
    if (!cur) throw std::invalid_argument("plain is not valid for encryption parameters");
    if (!target) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    if (!plain.is_ntt_form()) throw std::invalid_argument("plain is not in NTT form");
    if (cur->chain_index() < target->chain_index())
        throw std::invalid_argument("cannot switch to higher level modulus");
    if (plain.parms_id() == parms_id) return;
    const std::size_t L2 = target->parms().coeff_modulus().size();
    const double scale = plain.scale();
    plain.set_level(context_, parms_id, L2); // shrinking keeps the prefix limbs
    plain.scale() = scale;
}

void Evaluator::rescale_to_next(const Ciphertext &encrypted, Ciphertext &destination, MemoryPoolHandle) const
{
    TRACE_OP("rescale", trace::ct(destination), trace::ct(encrypted));
    // evaluator.cpp:1378-1414, mod_switch_scale_to_next :1118-1181
    const Rescale r = check_rescale(context_, encrypted);
    void *s = context_.stream();
    const std::size_t size = encrypted.size();
    Placed out(context_, Placed::fresh, encrypted, destination, size, r.lv.L - 1);
    const std::uint64_t *p = encrypted.store().dev_read(s);
    chk(mhe_rescale_to_next(context_.engine(), p, out.out(s), (int)size, (int)r.lv.L, s));
    out.commit(r.next, r.scale);
}

void Evaluator::rescale_to_next_inplace(Ciphertext &encrypted, MemoryPoolHandle) const
{
    if (merge_point([&] { return LsOp{ LsOp::RESC, {}, {}, {}, { &encrypted } }; })) return;
    rescale_to_next(encrypted, encrypted);
}

void Evaluator::rescale_to_inplace(Ciphertext &encrypted, parms_id_type parms_id, MemoryPoolHandle) const
{
    TRACE_OP("rescale", trace::ct(encrypted), trace::ct(encrypted));
    // evaluator.cpp:1416-1466
    Level target;
    check_target(context_, encrypted, parms_id, target);
    while (encrypted.parms_id() != parms_id) rescale_to_next(encrypted, encrypted);
}

void Evaluator::multiply_plain_inplace(Ciphertext &encrypted, const Plaintext &plain, MemoryPoolHandle) const
{
    multiply_plain(encrypted, plain, encrypted);
}

void Evaluator::multiply_plain(const Ciphertext &encrypted, const Plaintext &plain, Ciphertext &destination,
                               MemoryPoolHandle) const
{
    TRACE_OP("multiply_plain", trace::ct(destination), trace::ct(encrypted), trace::pt(plain));
    // evaluator.cpp:1726-1761, multiply_plain_ntt :1891-1930 (out of place: no copy of encrypted)
    Level lv = check_ct(context_, encrypted, "encrypted");
    if (plain.is_ntt_form()) level_of(context_, plain.parms_id(), "plain");
    if (encrypted.is_ntt_form() != plain.is_ntt_form()) throw std::invalid_argument("NTT form mismatch");
    if (!encrypted.is_ntt_form()) throw std::invalid_argument("encrypted must be in NTT form");
    if (encrypted.parms_id() != plain.parms_id())
        throw std::invalid_argument("encrypted_ntt and plain_ntt parameter mismatch");
    const double new_scale = encrypted.scale() * plain.scale();
    check_scale(new_scale, lv);
    void *s = context_.stream();
    const std::uint64_t *b = plain.store().dev_read(s);
    const std::size_t size = encrypted.size();
    Placed out = Placed::onto(context_, encrypted, destination, lv.L);
    const std::uint64_t *a = out.in(s);
    chk(mhe_multiply_plain(context_.engine(), a, b, out.out(s), (int)size, (int)lv.L, s));
    out.commit(encrypted.parms_id(), new_scale);
}

static void add_sub_plain(const SEALContext &ctx, Ciphertext &encrypted, const Plaintext &plain, bool sub)
{
    // evaluator.cpp:1578-1724 (CKKS branch): component 0 +-= plain
    Level lv = check_ct(ctx, encrypted, "encrypted");
    if (encrypted.is_ntt_form() != plain.is_ntt_form()) throw std::invalid_argument("NTT form mismatch");
    if (encrypted.parms_id() != plain.parms_id())
        throw std::invalid_argument("encrypted and plain parameter mismatch");
    if (!are_close(encrypted.scale(), plain.scale())) throw std::invalid_argument("scale mismatch");
    void *s = ctx.stream();
    const std::uint64_t *b = plain.store().dev_read(s);
    std::uint64_t *a = encrypted.store().dev_write(s);
    if (sub)
        chk(mhe_sub(ctx.engine(), a, b, a, 1, (int)lv.L, s));
    else
        chk(mhe_add(ctx.engine(), a, b, a, 1, (int)lv.L, s));
}

void Evaluator::add_plain_inplace(Ciphertext &encrypted, const Plaintext &plain) const
{
    TRACE_OP("add_plain", trace::ct(encrypted), trace::ct(encrypted), trace::pt(plain));
    add_sub_plain(context_, encrypted, plain, false);
}

void Evaluator::add_plain(const Ciphertext &encrypted, const Plaintext &plain, Ciphertext &destination) const
{
    TRACE_OP("add_plain", trace::ct(destination), trace::ct(encrypted), trace::pt(plain));
    destination = encrypted;
    add_plain_inplace(destination, plain);
}

void Evaluator::sub_plain_inplace(Ciphertext &encrypted, const Plaintext &plain) const
{
    TRACE_OP("sub_plain", trace::ct(encrypted), trace::ct(encrypted), trace::pt(plain));
    add_sub_plain(context_, encrypted, plain, true);
}

void Evaluator::sub_plain(const Ciphertext &encrypted, const Plaintext &plain, Ciphertext &destination) const
{
    TRACE_OP("sub_plain", trace::ct(destination), trace::ct(encrypted), trace::pt(plain));
    destination = encrypted;
    sub_plain_inplace(destination, plain);
}

void Evaluator::transform_to_ntt_inplace(Ciphertext &encrypted) const
{
    TRACE_OP("ntt_fwd", trace::ct(encrypted), trace::ct(encrypted));
    // evaluator.cpp:2025-2071
    Level lv = check_ct(context_, encrypted, "encrypted");
    if (encrypted.is_ntt_form()) throw std::invalid_argument("encrypted is already in NTT form");
    void *s = context_.stream();
    chk(mhe_ntt_forward(context_.engine(), encrypted.store().dev_write(s), (int)encrypted.size(), (int)lv.L, 0, s));
    encrypted.is_ntt_form() = true;
}

void Evaluator::transform_from_ntt_inplace(Ciphertext &encrypted) const
{
    TRACE_OP("ntt_inv", trace::ct(encrypted), trace::ct(encrypted));
    // evaluator.cpp:2073-2118
    Level lv = check_ct(context_, encrypted, "encrypted");
    if (!encrypted.is_ntt_form()) throw std::invalid_argument("encrypted is not in NTT form");
    void *s = context_.stream();
    chk(mhe_ntt_inverse(context_.engine(), encrypted.store().dev_write(s), (int)encrypted.size(), (int)lv.L, 0, s));
    encrypted.is_ntt_form() = false;
}

// apply_galois_inplace (evaluator.cpp:2120-2222) on destination's own words (in place: destination is
// encrypted), or reading encrypted and writing destination (which the engine refuses for one object)
static void galois(const SEALContext &ctx, const Ciphertext &encrypted, std::uint32_t galois_elt,
            const GaloisKeys &galois_keys, Ciphertext &destination, bool inplace)
{
    Level lv = check_galois(ctx, encrypted, galois_elt, galois_keys);
    void *s = ctx.stream();
    std::size_t kl = 0;
    const std::uint64_t *key = galois_keys.key_for(GaloisKeys::get_index(galois_elt), lv.L, s, kl);
    Placed out(ctx, inplace ? Placed::same : Placed::reuse, encrypted, destination, 2, lv.L);
    if (inplace)
        chk(mhe_apply_galois(ctx.engine(), out.out(s), galois_elt, key, (int)kl, (int)lv.L, s));
    else
    {
        const std::uint64_t *a = out.in(s);
        chk(mhe_apply_galois_to(ctx.engine(), a, out.out(s), galois_elt, key, (int)kl, (int)lv.L, s));
    }
}

void Evaluator::apply_galois_inplace(Ciphertext &encrypted, std::uint32_t galois_elt, const GaloisKeys &galois_keys,
                                     MemoryPoolHandle) const
{
    TRACE_OP("galois", trace::ct(encrypted), trace::ct(encrypted));
    TRACE_EXTRA("\"elt\": " + std::to_string(galois_elt));
    galois(context_, encrypted, galois_elt, galois_keys, encrypted, true);
}

void Evaluator::apply_galois_to(const Ciphertext &encrypted, std::uint32_t galois_elt, const GaloisKeys &galois_keys,
                                Ciphertext &destination) const
{
    TRACE_OP("galois", trace::ct(destination), trace::ct(encrypted));
    TRACE_EXTRA("\"elt\": " + std::to_string(galois_elt));
    galois(context_, encrypted, galois_elt, galois_keys, destination, false);
}

void Evaluator::rotate_internal(const Ciphertext &encrypted, int steps, const GaloisKeys &galois_keys,
                                Ciphertext &destination) const
{
    // evaluator.cpp:2224-2279.  Out of place a keyed step is written straight to the destination;
    // a zero step or a NAF-composed one works on a copy.
    const bool copy = &encrypted != &destination;
    if (copy && steps == 0) destination = encrypted;
    Level lv = level_of(context_, encrypted.parms_id(), "encrypted");
    check_key_parms(context_, galois_keys, "galois_keys");
    if (steps == 0) return;
    const StepKey k = step_key(lv.n, steps, galois_keys);
    if (k.has_key && copy) return apply_galois_to(encrypted, k.elt, galois_keys, destination);
    if (k.has_key) return apply_galois_inplace(destination, k.elt, galois_keys);
    if (copy) destination = encrypted;
    // NAF decomposition (util/numth.h:22-42)
    std::vector<int> naf;
    const bool sign = steps < 0;
    int v = std::abs(steps);
    for (int i = 0; v; i++)
    {
        const int zi = (v & 1) ? 2 - (v & 3) : 0;
        v = (v - zi) >> 1;
        if (zi) naf.push_back((sign ? -zi : zi) * (1 << i));
    }
    if (naf.size() == 1) throw std::invalid_argument("Galois key not present");
    for (int st : naf)
        if ((std::size_t)std::abs(st) != (lv.n >> 1)) rotate_internal(destination, st, galois_keys, destination);
}

void Evaluator::rotate_vector_inplace(Ciphertext &encrypted, int steps, const GaloisKeys &galois_keys,
                                      MemoryPoolHandle) const
{
    rotate_vector(encrypted, steps, galois_keys, encrypted);
}

void Evaluator::rotate_vector(const Ciphertext &encrypted, int steps, const GaloisKeys &galois_keys,
                              Ciphertext &destination, MemoryPoolHandle) const
{
    const auto op = [&] { return LsOp{ LsOp::ROT, { &encrypted }, {}, { steps }, { &destination }, &galois_keys }; };
    if (merge_point(op)) return;
    TRACE_OP("rotate", trace::ct(destination), trace::ct(encrypted));
    TRACE_EXTRA("\"step\": " + std::to_string(steps));
    rotate_internal(encrypted, steps, galois_keys, destination);
}

void Evaluator::complex_conjugate_inplace(Ciphertext &encrypted, const GaloisKeys &galois_keys, MemoryPoolHandle) const
{
    complex_conjugate(encrypted, galois_keys, encrypted);
}

void Evaluator::complex_conjugate(const Ciphertext &encrypted, const GaloisKeys &galois_keys, Ciphertext &destination,
                                  MemoryPoolHandle) const
{
    TRACE_OP("galois", trace::ct(destination), trace::ct(encrypted));
    TRACE_EXTRA("\"elt\": " + std::to_string(2 * encrypted.poly_modulus_degree() - 1));
    const std::size_t n = level_of(context_, encrypted.parms_id(), "encrypted").n;
    if (&encrypted == &destination)
        apply_galois_inplace(destination, (std::uint32_t)(2 * n - 1), galois_keys);
    else
        apply_galois_to(encrypted, (std::uint32_t)(2 * n - 1), galois_keys, destination);
}

// ---- modified SEAL entry points (evaluator.cpp:287-486) ------------------------------------
void Evaluator::add_const_inplace(Ciphertext &encrypted, double value) const { add_const(encrypted, value, encrypted); }

void Evaluator::add_const(const Ciphertext &encrypted, double value, Ciphertext &destination) const
{
    TRACE_OP("add_const", trace::ct(destination), trace::ct(encrypted));
    TRACE_EXTRA("\"value\": " + trace::num(value));
    Level lv;
    const std::vector<std::uint64_t> r = scalar_residues(context_, encrypted, value, lv);
    void *s = context_.stream();
    const std::size_t pw = lv.L * lv.n, size = encrypted.size();
    Placed out = Placed::onto(context_, encrypted, destination, lv.L);
    const std::uint64_t *a = out.in(s);
    std::uint64_t *d = out.out(s);
    chk(mhe_add_scalar(context_.engine(), a, r.data(), d, 1, (int)lv.L, s));
    // the constant goes to component 0; out of place the others are copied
    if (a != d && size > 1) chk(mhe_memcpy_d2d(context_.engine(), d + pw, a + pw, (size - 1) * pw * 8, s));
}

void Evaluator::multiply_const_inplace(Ciphertext &encrypted, double value) const
{
    multiply_const(encrypted, value, encrypted);
}

void Evaluator::multiply_const(const Ciphertext &encrypted, double value, Ciphertext &destination) const
{
    TRACE_OP("multiply_const", trace::ct(destination), trace::ct(encrypted));
    TRACE_EXTRA("\"value\": " + trace::num(value));
    Level lv;
    const std::vector<std::uint64_t> r = scalar_residues(context_, encrypted, value, lv);
    const double new_scale = encrypted.scale() * encrypted.scale();
    check_scale(new_scale, lv);
    void *s = context_.stream();
    const std::size_t size = encrypted.size();
    Placed out = Placed::onto(context_, encrypted, destination, lv.L);
    const std::uint64_t *a = out.in(s);
    chk(mhe_multiply_scalar(context_.engine(), a, r.data(), out.out(s), (int)size, (int)lv.L, s));
    out.commit(encrypted.parms_id(), new_scale);
}

// one term encrypted * plain of a fused product sum whose accumulator has acc_limbs limbs, acc_size
// components and the form acc_ntt: the product's scale
static double check_plain_term(const Ciphertext &encrypted, const Plaintext &plain, const Level &lv, std::size_t acc_limbs,
                        std::size_t acc_size, bool acc_ntt)
{
    if (acc_limbs != lv.L || acc_size != encrypted.size())
        throw std::invalid_argument("multiply_plain_add: acc and encrypted must share level and size");
    if (!encrypted.is_ntt_form() || !plain.is_ntt_form() || !acc_ntt) throw std::invalid_argument("NTT form mismatch");
    if (encrypted.parms_id() != plain.parms_id())
        throw std::invalid_argument("encrypted_ntt and plain_ntt parameter mismatch");
    const double new_scale = encrypted.scale() * plain.scale();
    check_scale(new_scale, lv);
    return new_scale;
}

void Evaluator::multiply_plain_add_reduced_error(Ciphertext &acc, const Ciphertext &encrypted,
                                                 const Plaintext &plain) const
{
    TRACE_OP("multiply_plain_add", trace::ct(acc), trace::ct(acc), trace::ct(encrypted), trace::pt(plain));
    // multiply_plain(encrypted, plain, tmp) + add_inplace_reduced_error(acc, tmp) at equal levels,
    // one kernel (bit-identical): acc takes the product's scale, as the reduced-error add assigns it
    Level lv = check_ct(context_, encrypted, "encrypted");
    Level la = check_ct(context_, acc, "encrypted1");
    const double new_scale = check_plain_term(encrypted, plain, lv, la.L, acc.size(), acc.is_ntt_form());
    void *s = context_.stream();
    const std::uint64_t *b = plain.store().dev_read(s);
    const std::uint64_t *a = encrypted.store().dev_read(s);
    chk(mhe_multiply_plain_add(context_.engine(), a, b, acc.store().dev_write(s), (int)encrypted.size(), (int)lv.L, s));
    acc.scale() = new_scale;
}

void Evaluator::multiply_plain_sum(const std::vector<const Ciphertext *> &encrypted,
                                   const std::vector<const Plaintext *> &plain, Ciphertext &destination) const
{
    if (encrypted.empty() || encrypted.size() != plain.size())
        throw std::invalid_argument("encrypted and plain must be non-empty and of the same size");
    for (std::size_t k = 0; k < encrypted.size(); k++)
        if (!encrypted[k] || !plain[k] || encrypted[k] == &destination)
            throw std::invalid_argument("multiply_plain_sum: null operand or destination among the inputs");
    // term by term under the evaluator trace (one record per operation) or with batching off
    if (trace::enabled() || !batched_launches())
    {
        multiply_plain(*encrypted[0], *plain[0], destination);
        for (std::size_t k = 1; k < encrypted.size(); k++)
            multiply_plain_add_reduced_error(destination, *encrypted[k], *plain[k]);
        return;
    }
    const Ciphertext &e0 = *encrypted[0];
    Level lv = check_ct(context_, e0, "encrypted");
    double new_scale = 0;
    for (std::size_t k = 0; k < encrypted.size(); k++)
    {
        const Ciphertext &e = *encrypted[k];
        const Plaintext &p = *plain[k];
        new_scale = check_plain_term(e, p, check_ct(context_, e, "encrypted"), lv.L, e0.size(), true);
    }
    void *s = context_.stream();
    std::vector<const std::uint64_t *> a, b;
    for (std::size_t k = 0; k < encrypted.size(); k++)
    {
        a.push_back(encrypted[k]->store().dev_read(s));
        b.push_back(plain[k]->store().dev_read(s));
    }
    fresh_dest(context_, e0, destination, e0.size());
    chk(mhe_multiply_plain_sum(context_.engine(), (int)a.size(), a.data(), b.data(), destination.store().dev_write(s, true),
                               0, (int)e0.size(), (int)lv.L, s));
    destination.scale() = new_scale; // the last term's product scale, as the reduced-error adds leave it
}

// real and imaginary parts (im stays empty for real values)
template <typename T>
static void split(const std::vector<T> &v, std::vector<double> &re, std::vector<double> &im)
{
    for (const T &x : v)
    {
        re.push_back(std::real(x));
        if constexpr (!std::is_same_v<T, double>) im.push_back(std::imag(x));
    }
}

template <typename T>
void Evaluator::multiply_vector_inplace(Ciphertext &encrypted, const std::vector<T> &value) const
{
    // evaluator.cpp:303-310: encode at the first level, mod_switch_to, multiply_plain
    Plaintext plain;
    encode_vector_for(encrypted, value, plain);
    multiply_plain_inplace(encrypted, plain);
}

template <typename T>
void Evaluator::encode_vector_for(const Ciphertext &encrypted, const std::vector<T> &value, Plaintext &plain) const
{
    // CKKSEncoder::encode(value, encrypted.scale()) at the first level, then mod_switch_to the
    // ciphertext's level: only the kept limbs are produced (SEAL's bounds are checked at the
    // first level)
    Level lv = check_ct(context_, encrypted, "encrypted");
    const std::size_t L1 = context_.first_context_data()->parms().coeff_modulus().size();
    if (value.size() > lv.n / 2) throw std::invalid_argument("values_size is too large");
    std::vector<double> re, im;
    split<T>(value, re, im);
    TRACE_OP("encode_for", trace::pt(plain), trace::vec(re.data(), im.empty() ? nullptr : im.data(), re.size()));
    TRACE_EXTRA("\"scale\": " + trace::num(encrypted.scale()) + ", \"limbs\": " + std::to_string(lv.L));
    void *s = context_.stream();
    plain.set_level(context_, encrypted.parms_id(), lv.L);
    plain.scale() = encrypted.scale();
    chk(mhe_ckks_encode_at(context_.engine(), encoder_.handle(), re.data(), im.empty() ? nullptr : im.data(),
                           re.size(), encrypted.scale(), (int)L1, (int)lv.L, plain.store().dev_write(s, true), s));
}

using cvector = std::vector<std::complex<double>>;
template void Evaluator::encode_vector_for<double>(const Ciphertext &, const std::vector<double> &, Plaintext &) const;
template void Evaluator::encode_vector_for<std::complex<double>>(const Ciphertext &, const cvector &, Plaintext &) const;
template void Evaluator::multiply_vector_inplace<double>(Ciphertext &, const std::vector<double> &) const;
template void Evaluator::multiply_vector_inplace<std::complex<double>>(Ciphertext &, const cvector &) const;

// evaluator.cpp:312-486 (Kim et al., CT-RSA 2022): when the levels differ, the operand at the
// higher level is multiplied by s_other * q_last / s^2 (multiply_const), its scale forced to
// s_other * q_last, rescaled and mod-switched down to the other operand's level; equal levels
// only copy the scale across.  Same operation order and scale assignments as the reference.
void Evaluator::reduced_error_op(Ciphertext &encrypted1, const Ciphertext &encrypted2, Rmode mode) const
{
    auto op_inplace = [&](Ciphertext &a, const Ciphertext &b) {
        mode == Rmode::add ? add_inplace(a, b) : mode == Rmode::sub ? sub_inplace(a, b) : multiply_inplace(a, b);
    };
    auto op_out = [&](const Ciphertext &a, const Ciphertext &b, Ciphertext &d) {
        mode == Rmode::add ? add(a, b, d) : mode == Rmode::sub ? sub(a, b, d) : multiply(a, b, d);
    };
    // the higher operand brought down to the other's level, its scale as the rescale leaves it
    auto adjusted = [&](const Ciphertext &high, const char *what, const Ciphertext &low, Ciphertext &adj) {
        const double q = static_cast<double>(level_of(context_, high.parms_id(), what)
                                                 .cd->parms()
                                                 .coeff_modulus()[high.coeff_modulus_size() - 1]
                                                 .value());
        const double scale_adjust = low.scale() * q / (high.scale() * high.scale());
        multiply_const(high, scale_adjust, adj);
        adj.scale() = low.scale() * q;
        rescale_to_next_inplace(adj);
        mod_switch_to_inplace(adj, low.parms_id());
    };
    const std::size_t l1 = encrypted1.coeff_modulus_size(), l2 = encrypted2.coeff_modulus_size();
    if (l1 == l2)
    {
        encrypted1.scale() = encrypted2.scale();
        op_inplace(encrypted1, encrypted2);
    }
    else if (l1 < l2)
    {
        Ciphertext adj;
        adjusted(encrypted2, "encrypted2", encrypted1, adj);
        encrypted1.scale() = adj.scale();
        op_inplace(encrypted1, adj);
    }
    else
    {
        Ciphertext adj;
        adjusted(encrypted1, "encrypted1", encrypted2, adj);
        adj.scale() = encrypted2.scale();
        op_out(adj, encrypted2, encrypted1);
    }
}

void Evaluator::reduced_error_out(const Ciphertext &encrypted1, const Ciphertext &encrypted2, Ciphertext &destination,
                                  Rmode mode, const RelinKeys *relin_keys) const
{
    const auto op = [&] {
        return LsOp{ LsOp::MULRE, { &encrypted1 }, { &encrypted2 }, {}, { &destination }, nullptr, relin_keys };
    };
    // pinned, not endorsed: this merge point alone submits inside a Lockstep group only, not in a fiber
    if (mode == Rmode::mul && merge_point(op, true)) return;
    TRACE_OP(mode == Rmode::add ? "add_re" : mode == Rmode::sub ? "sub_re" : "mul_re", trace::ct(destination),
             trace::ct(encrypted1), trace::ct(encrypted2));
    // equal levels: encrypted1 takes encrypted2's scale, then the op (reduced_error_op); written
    // out of place so encrypted1 is not copied first
    const bool same = encrypted1.coeff_modulus_size() == encrypted2.coeff_modulus_size() &&
                      encrypted1.parms_id() == encrypted2.parms_id() && encrypted1.size() == encrypted2.size() &&
                      encrypted1.size() == 2 && &encrypted1 != &destination && &encrypted2 != &destination;
    if (!same)
    {
        destination = encrypted1;
        reduced_error_op(destination, encrypted2, mode);
        if (mode == Rmode::mul) relinearize_inplace(destination, *relin_keys);
        return;
    }
    if (mode == Rmode::mul)
    {
        mulre_product(context_, encrypted1, encrypted2, destination);
        relinearize_inplace(destination, *relin_keys);
        return;
    }
    check_pair(context_, encrypted1, encrypted2, false);
    void *s = context_.stream();
    const Level lv = level_of(context_, encrypted1.parms_id(), "encrypted1");
    const std::uint64_t *a = encrypted1.store().dev_read(s), *b = encrypted2.store().dev_read(s);
    fresh_dest(context_, encrypted1, destination, 2);
    std::uint64_t *d = destination.store().dev_write(s, true);
    if (mode == Rmode::add)
        chk(mhe_add(context_.engine(), a, b, d, 2, (int)lv.L, s));
    else
        chk(mhe_sub(context_.engine(), a, b, d, 2, (int)lv.L, s));
    destination.scale() = encrypted2.scale();
}

void Evaluator::add_inplace_reduced_error(Ciphertext &encrypted1, const Ciphertext &encrypted2) const
{
    TRACE_OP("add_re", trace::ct(encrypted1), trace::ct(encrypted1), trace::ct(encrypted2));
    reduced_error_op(encrypted1, encrypted2, Rmode::add);
}

void Evaluator::sub_inplace_reduced_error(Ciphertext &encrypted1, const Ciphertext &encrypted2) const
{
    TRACE_OP("sub_re", trace::ct(encrypted1), trace::ct(encrypted1), trace::ct(encrypted2));
    reduced_error_op(encrypted1, encrypted2, Rmode::sub);
}

void Evaluator::multiply_inplace_reduced_error(Ciphertext &encrypted1, const Ciphertext &encrypted2,
                                               const RelinKeys &relin_keys) const
{
    const auto op = [&] {
        return LsOp{ LsOp::MULRE, { &encrypted1 }, { &encrypted2 }, {}, { &encrypted1 }, nullptr, &relin_keys };
    };
    if (merge_point(op)) return;
    TRACE_OP("mul_re", trace::ct(encrypted1), trace::ct(encrypted1), trace::ct(encrypted2));
    reduced_error_op(encrypted1, encrypted2, Rmode::mul);
    relinearize_inplace(encrypted1, relin_keys);
}
} // namespace seal
