// context.cpp -- encryption parameters, the modulus switching chain (SEALContext) and the per-thread
// engine streams, after SEAL's context.cpp, encryptionparams.cpp and modulus.cpp; also the basics
// every unit uses (seal_internal.h): the engine-error mapping, are_close, the PRNG factory.
#include "seal_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <map>
#include <mutex>
#include <thread>
#include <unordered_map>

namespace seal
{
const parms_id_type parms_id_zero = { 0, 0, 0, 0 };

[[noreturn]] void raise(int rc)
{
    const std::string msg = mhe_last_error();
    switch (rc)
    {
    case MHE_ERR_ARG: throw std::invalid_argument(msg);
    case MHE_ERR_RANGE:
        if (msg.find("out of range") != std::string::npos) throw std::out_of_range(msg);
        throw std::invalid_argument(msg);
    default: throw std::runtime_error(msg);
    }
}

// util::are_close (util/common.h): |a-b| < eps * max(|a|, |b|, 1)
bool are_close(double a, double b)
{
    const double scale = std::max({ std::fabs(a), std::fabs(b), 1.0 });
    return std::fabs(a - b) < std::numeric_limits<double>::epsilon() * scale;
}

static int product_bits(const std::vector<Modulus> &cm, std::size_t count)
{
    std::vector<std::uint64_t> prod(count + 1, 0);
    prod[0] = 1;
    std::size_t words = 1;
    for (std::size_t j = 0; j < count; j++)
    {
        std::uint64_t carry = 0;
        for (std::size_t w = 0; w < words; w++)
        {
            const unsigned __int128 t = (unsigned __int128)prod[w] * cm[j].value() + carry;
            prod[w] = (std::uint64_t)t;
            carry = (std::uint64_t)(t >> 64);
        }
        if (carry) prod[words++] = carry;
    }
    return (int)(64 * (words - 1)) + (64 - __builtin_clzll(prod[words - 1]));
}

// the factory key generation and encryption draw their PRNGs from (SEAL: the context installs
// DefaultFactory when the parameters carry none, context.cpp:464-467)
std::shared_ptr<UniformRandomGeneratorFactory> factory_of(const SEALContext &ctx)
{
    return ctx.key_context_data()->parms().random_generator_or_default();
}

std::vector<std::uint64_t> moduli_of(const SEALContext &ctx)
{
    std::vector<std::uint64_t> q;
    for (auto &m : ctx.key_context_data()->parms().coeff_modulus()) q.push_back(m.value());
    return q;
}

// ------------------------------------------------------------------------------ Modulus
int Modulus::bit_count() const noexcept
{
    return value_ ? 64 - __builtin_clzll(value_) : 0;
}

std::vector<Modulus> CoeffModulus::Create(std::size_t poly_modulus_degree, std::vector<int> bit_sizes)
{
    std::vector<std::uint64_t> out(bit_sizes.size());
    chk(mhe_coeff_modulus_create(poly_modulus_degree, bit_sizes.data(), (int)bit_sizes.size(), out.data()));
    return std::vector<Modulus>(out.begin(), out.end());
}

parms_id_type blake2b_parms_id(const std::uint64_t *words, std::size_t count); // serialize.cpp

parms_id_type EncryptionParameters::parms_id() const
{
    // SEAL's parms_id (encryptionparams.cpp:124-158): BLAKE2b-256 of [scheme, n, coeff moduli...,
    // plain modulus] as u64 words; the CKKS plain modulus is the zero Modulus (one word)
    std::vector<std::uint64_t> w{ (std::uint64_t)scheme_, (std::uint64_t)n_ };
    for (auto &m : coeff_modulus_) w.push_back(m.value());
    w.push_back(0);
    return blake2b_parms_id(w.data(), w.size());
}

// ------------------------------------------------------------------------------ SEALContext
struct SEALContext::Impl : std::enable_shared_from_this<SEALContext::Impl>
{
    EncryptionParameters parms;
    std::vector<std::shared_ptr<ContextData>> levels; // by number of primes - 1
    std::map<parms_id_type, std::shared_ptr<const ContextData>> by_id;
    std::shared_ptr<const ContextData> key, first, last;
    mhe_ctx *eng = nullptr;
    std::size_t K = 0;
    sec_level_type sec_level = sec_level_type::tc128;
    bool insecure = false;
    std::mutex mu;
    std::unordered_map<std::thread::id, void *> streams;
    // streams of threads that have exited: the next new thread takes one instead of creating a
    // stream (and with it a scratch workspace) of its own.  A stream is never destroyed while the
    // context lives -- objects written on it keep it as their writer -- so without the pool a
    // process that starts threads per batch (the reference's OpenMP team, ResNetRunner::infer_batch)
    // would grow one workspace per thread it ever ran.
    std::vector<void *> idle;

    // the calling thread's leases: on thread exit each still-living context gets the stream back
    struct Leases
    {
        std::vector<std::weak_ptr<Impl>> ctx;
        ~Leases()
        {
            const auto id = std::this_thread::get_id();
            for (auto &w : ctx)
                if (auto p = w.lock()) p->release(id);
        }
    };

    void release(std::thread::id id)
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = streams.find(id);
        if (it == streams.end()) return;
        idle.push_back(it->second);
        streams.erase(it);
    }

    void *stream()
    {
        static thread_local Leases leases;
        std::lock_guard<std::mutex> g(mu);
        auto it = streams.find(std::this_thread::get_id());
        if (it != streams.end()) return it->second;
        void *s = nullptr;
        if (!idle.empty())
        {
            s = idle.back(); // ordered after its previous thread's work: same stream
            idle.pop_back();
        }
        else
            chk(mhe_stream_create(eng, &s));
        streams.emplace(std::this_thread::get_id(), s);
        leases.ctx.push_back(weak_from_this());
        return s;
    }

    ~Impl()
    {
        for (auto &kv : streams) idle.push_back(kv.second);
        for (void *s : idle)
        {
            (void)mhe_stream_sync(eng, s);
            (void)mhe_stream_destroy(eng, s);
        }
        if (eng) (void)mhe_ctx_destroy(eng);
    }
};

namespace
{
// CoeffModulus::MaxBitCount (modulus.cpp:112-116, util/hestdparms.h: HomomorphicEncryption.org
// classical tables; the modified SEAL adds 65536 -> 1792 for tc128)
int max_bit_count(std::size_t n, sec_level_type sec)
{
    static const std::map<std::size_t, int> tc128{ { 1024, 27 },   { 2048, 54 },   { 4096, 109 },  { 8192, 218 },
                                                   { 16384, 438 }, { 32768, 881 }, { 65536, 1792 } };
    static const std::map<std::size_t, int> tc192{ { 1024, 19 }, { 2048, 37 }, { 4096, 75 },
                                                   { 8192, 152 }, { 16384, 305 }, { 32768, 611 } };
    static const std::map<std::size_t, int> tc256{ { 1024, 14 }, { 2048, 29 }, { 4096, 58 },
                                                   { 8192, 118 }, { 16384, 237 }, { 32768, 476 } };
    const std::map<std::size_t, int> *t = sec == sec_level_type::tc128   ? &tc128
                                          : sec == sec_level_type::tc192 ? &tc192
                                          : sec == sec_level_type::tc256 ? &tc256
                                                                         : nullptr;
    if (!t) return std::numeric_limits<int>::max();
    auto it = t->find(n);
    return it == t->end() ? 0 : it->second;
}
} // namespace

int CoeffModulus::MaxBitCount(std::size_t poly_modulus_degree, sec_level_type sec_level) noexcept
{
    const int m = max_bit_count(poly_modulus_degree, sec_level);
    return m == std::numeric_limits<int>::max() ? 0 : m;
}

SEALContext::SEALContext(const EncryptionParameters &parms, bool expand_mod_chain, sec_level_type sec_level)
{
    if (parms.scheme() != scheme_type::ckks) throw std::invalid_argument("unsupported scheme");
    const auto &cm = parms.coeff_modulus();
    const std::size_t n = parms.poly_modulus_degree();
    if (cm.empty()) throw std::invalid_argument("coeff_modulus is not set");
    if (!n || (n & (n - 1))) throw std::invalid_argument("poly_modulus_degree is not a power of two");
    int log_n = 0;
    while ((std::size_t(1) << log_n) < n) log_n++;

    auto impl = std::make_shared<Impl>();
    impl->parms = parms;
    impl->K = cm.size();
    // context.cpp:207-220: parameters above the HomomorphicEncryption.org bound for the requested
    // security level are kept but flagged; key generators, encryptors, ... then refuse them
    impl->sec_level = sec_level;
    if (product_bits(cm, cm.size()) > max_bit_count(n, sec_level)) impl->insecure = true;
    std::vector<std::uint64_t> q;
    for (auto &m : cm) q.push_back(m.value());
    int device = 0;
    if (const char *d = std::getenv("MHE_DEVICE")) device = std::atoi(d);
    chk(mhe_ctx_create(&impl->eng, log_n, q.data(), (int)q.size(), device));

    // context.cpp: key level (all primes) -> first (drop the special prime) -> ... -> one prime
    const std::size_t K = impl->K;
    impl->levels.resize(K);
    auto make_level = [&](std::size_t count) {
        auto cd = std::make_shared<ContextData>();
        cd->parms_ = parms;
        cd->parms_.set_coeff_modulus(std::vector<Modulus>(cm.begin(), cm.begin() + count));
        cd->parms_id_ = cd->parms_.parms_id();
        cd->total_bits_ = product_bits(cm, count);
        impl->levels[count - 1] = cd;
        impl->by_id[cd->parms_id_] = cd;
        return cd;
    };
    auto key = make_level(K);
    impl->key = key;
    if (K == 1)
    {
        key->chain_index_ = 0;
        impl->first = impl->last = key;
    }
    else
    {
        key->chain_index_ = K - 1;
        std::shared_ptr<ContextData> prev = key;
        const std::size_t lowest = expand_mod_chain ? 1 : K - 1;
        for (std::size_t c = K - 1; c >= lowest; c--)
        {
            auto cd = make_level(c);
            cd->chain_index_ = c - 1;
            cd->prev_ = prev;
            prev->next_ = cd;
            if (c == K - 1) impl->first = cd;
            impl->last = cd;
            prev = cd;
            if (c == 1) break;
        }
    }
    impl_ = impl;
}

std::shared_ptr<const SEALContext::ContextData> SEALContext::get_context_data(const parms_id_type &id) const
{
    auto it = impl_->by_id.find(id);
    return it == impl_->by_id.end() ? nullptr : it->second;
}
std::shared_ptr<const SEALContext::ContextData> SEALContext::key_context_data() const { return impl_->key; }
std::shared_ptr<const SEALContext::ContextData> SEALContext::first_context_data() const { return impl_->first; }
std::shared_ptr<const SEALContext::ContextData> SEALContext::last_context_data() const { return impl_->last; }
const parms_id_type &SEALContext::key_parms_id() const { return impl_->key->parms_id(); }
const parms_id_type &SEALContext::first_parms_id() const { return impl_->first->parms_id(); }
const parms_id_type &SEALContext::last_parms_id() const { return impl_->last->parms_id(); }
bool SEALContext::parameters_set() const noexcept { return impl_ && impl_->eng && !impl_->insecure; }
sec_level_type SEALContext::sec_level() const noexcept
{
    return impl_ && !impl_->insecure ? impl_->sec_level : sec_level_type::none;
}

void require_set(const SEALContext &ctx)
{
    if (!ctx.parameters_set()) throw std::invalid_argument("encryption parameters are not set correctly");
}
bool SEALContext::using_keyswitching() const noexcept { return impl_ && impl_->K > 1; }
mhe_ctx *SEALContext::engine() const { return impl_->eng; }
void *SEALContext::stream() const { return impl_->stream(); }
std::size_t SEALContext::key_size() const { return impl_->K; }
std::shared_ptr<void> SEALContext::handle() const { return impl_; }
void *SEALContext::stream_of(void *handle) { return static_cast<Impl *>(handle)->stream(); }
} // namespace seal
