// store.cpp -- PolyStore (device words with a host mirror and cross-stream ordering,
// stream_order.h), and the Ciphertext / Plaintext bookkeeping over it (ciphertext.h, plaintext.h).
#include "seal_internal.h"
#include "stream_order.h"

#include <algorithm>
#include <mutex>

namespace seal
{
// ------------------------------------------------------------------------------ PolyStore
void PolyStore::bind(const SEALContext &ctx)
{
    if (eng_ == ctx.engine()) return;
    release();
    hold_ = ctx.handle();
    eng_ = ctx.engine();
}

void *PolyStore::thread_stream() const
{
    if (!hold_) throw std::logic_error("polynomial storage is not bound to a context");
    return SEALContext::stream_of(hold_.get());
}

// Cross-stream ordering (stream_order.h): device-side waits, no host blocking.
void PolyStore::wait_writer(void *s) const
{
    for (void *w : detail::order_before<void *>(s, writer_, writer_done_, {}, detail::Access::read))
        chk(mhe_stream_wait(eng_, s, w));
}

void PolyStore::wait_all(void *s) const
{
    for (void *w : detail::order_before<void *>(s, writer_, writer_done_, readers_, detail::Access::write))
        chk(mhe_stream_wait(eng_, s, w));
    readers_.clear();
}

void PolyStore::release()
{
    if (dev_)
    {
        std::lock_guard<std::mutex> g(*mu_);
        void *s = writer_ ? writer_ : thread_stream();
        for (void *w : detail::order_before<void *>(s, writer_, writer_done_, readers_, detail::Access::release))
            (void)mhe_stream_wait(eng_, s, w);
        (void)mhe_free_async(eng_, dev_, s);
    }
    dev_ = nullptr;
    cap_ = 0;
    readers_.clear();
    writer_ = nullptr;
    writer_done_ = true;
}

PolyStore::~PolyStore()
{
    release();
}

void PolyStore::resize_words(std::size_t words, bool preserve)
{
    if (!eng_) throw std::logic_error("polynomial storage is not bound to a context");
    if (words <= cap_ || (!dev_valid_ && host_valid_))
    {
        words_ = words;
        if (host_valid_ && host_.size() < words) host_.resize(words, 0);
        if (!dev_valid_ && host_valid_ && words > cap_ && dev_)
        {
            // host is the authority: the device copy is reallocated on the next upload
            std::lock_guard<std::mutex> g(*mu_);
            void *s = thread_stream();
            wait_all(s);
            (void)mhe_free_async(eng_, dev_, s);
            dev_ = nullptr;
            cap_ = 0;
        }
        return;
    }
    void *s = thread_stream();
    std::lock_guard<std::mutex> g(*mu_);
    wait_all(s);
    void *p = nullptr;
    chk(mhe_malloc_async(eng_, &p, words * sizeof(std::uint64_t), s));
    if (preserve && dev_ && words_) chk(mhe_memcpy_d2d(eng_, p, dev_, std::min(words_, words) * 8, s));
    if (dev_) (void)mhe_free_async(eng_, dev_, s);
    dev_ = static_cast<std::uint64_t *>(p);
    cap_ = words;
    words_ = words;
    writer_ = s;
    writer_done_ = false;
    dev_valid_ = true;
    // the device copy is authoritative from here on; a host mirror is only kept when it already
    // held data (a fresh store would otherwise zero-fill a host vector of the full size)
    if (preserve && host_valid_ && !host_.empty())
        host_.resize(words, 0);
    else
    {
        host_valid_ = false;
        host_.clear();
    }
}

const std::uint64_t *PolyStore::dev_read(void *s) const
{
    if (!eng_) throw std::logic_error("polynomial storage is not bound to a context");
    std::lock_guard<std::mutex> g(*mu_);
    if (!dev_valid_)
    {
        auto *self = const_cast<PolyStore *>(this);
        if (!dev_ || cap_ < words_)
        {
            wait_all(s);
            if (dev_) (void)mhe_free_async(eng_, dev_, s);
            void *p = nullptr;
            chk(mhe_malloc_async(eng_, &p, words_ * sizeof(std::uint64_t), s));
            self->dev_ = static_cast<std::uint64_t *>(p);
            self->cap_ = words_;
        }
        wait_all(s);
        chk(mhe_memcpy_h2d(eng_, dev_, host_.data(), words_ * 8, s));
        chk(mhe_stream_sync(eng_, s));
        dev_valid_ = true;
        writer_ = s;
        writer_done_ = true;
    }
    if (writer_ != s && std::find(readers_.begin(), readers_.end(), s) == readers_.end())
    {
        wait_writer(s); // once per (write, reading stream): the stream is then ordered after it
        readers_.push_back(s);
    }
    return dev_;
}

std::uint64_t *PolyStore::dev_write(void *s, bool overwrite)
{
    if (!eng_) throw std::logic_error("polynomial storage is not bound to a context");
    if (!dev_valid_)
    {
        if (overwrite)
        {
            std::lock_guard<std::mutex> g(*mu_);
            if (!dev_ || cap_ < words_)
            {
                wait_all(s);
                if (dev_) (void)mhe_free_async(eng_, dev_, s);
                void *p = nullptr;
                chk(mhe_malloc_async(eng_, &p, words_ * sizeof(std::uint64_t), s));
                dev_ = static_cast<std::uint64_t *>(p);
                cap_ = words_;
            }
            dev_valid_ = true;
        }
        else
            (void)dev_read(s);
    }
    std::lock_guard<std::mutex> g(*mu_);
    wait_all(s);
    writer_ = s;
    writer_done_ = false;
    host_valid_ = false;
    return dev_;
}

const std::uint64_t *PolyStore::host() const
{
    if (!host_valid_)
    {
        std::lock_guard<std::mutex> g(*mu_);
        void *s = writer_ ? writer_ : thread_stream();
        host_.resize(words_);
        if (words_)
        {
            chk(mhe_memcpy_d2h(eng_, host_.data(), dev_, words_ * 8, s));
            chk(mhe_stream_sync(eng_, s));
        }
        writer_done_ = true;
        host_valid_ = true;
    }
    return host_.data();
}

std::uint64_t *PolyStore::host()
{
    const PolyStore *c = this;
    c->host();
    if (eng_)
    {
        std::lock_guard<std::mutex> g(*mu_);
        for (void *r : readers_) chk(mhe_stream_sync(eng_, r));
        readers_.clear();
        dev_valid_ = false;
    }
    return host_.data();
}

void PolyStore::copy_from(const PolyStore &o)
{
    hold_ = o.hold_;
    eng_ = o.eng_;
    words_ = o.words_;
    if (!eng_ || (!o.dev_valid_ && o.host_valid_))
    {
        host_ = o.host_;
        host_valid_ = true;
        dev_valid_ = !eng_;
        return;
    }
    void *s = thread_stream();
    const std::uint64_t *src = o.dev_read(s);
    void *p = nullptr;
    chk(mhe_malloc_async(eng_, &p, std::max<std::size_t>(words_, 1) * 8, s));
    if (words_) chk(mhe_memcpy_d2d(eng_, p, src, words_ * 8, s));
    dev_ = static_cast<std::uint64_t *>(p);
    cap_ = words_;
    writer_ = s;
    writer_done_ = false;
    dev_valid_ = true;
    host_valid_ = false;
}

PolyStore::PolyStore(const PolyStore &o)
{
    copy_from(o);
}

PolyStore &PolyStore::operator=(const PolyStore &o)
{
    if (this == &o) return *this;
    if (eng_ && eng_ == o.eng_ && dev_ && cap_ >= o.words_ && (o.dev_valid_ || !o.host_valid_))
    {
        // same engine, enough room: copy in place on this thread's stream
        void *s = thread_stream();
        const std::uint64_t *src = o.dev_read(s);
        std::uint64_t *dst = dev_write(s, true);
        words_ = o.words_;
        if (words_) chk(mhe_memcpy_d2d(eng_, dst, src, words_ * 8, s));
        return *this;
    }
    release();
    copy_from(o);
    return *this;
}

PolyStore::PolyStore(PolyStore &&o) noexcept
{
    *this = std::move(o);
}

PolyStore &PolyStore::operator=(PolyStore &&o) noexcept
{
    if (this == &o) return *this;
    std::swap(hold_, o.hold_);
    std::swap(eng_, o.eng_);
    std::swap(dev_, o.dev_);
    std::swap(words_, o.words_);
    std::swap(cap_, o.cap_);
    std::swap(host_, o.host_);
    std::swap(host_valid_, o.host_valid_);
    std::swap(dev_valid_, o.dev_valid_);
    std::swap(mu_, o.mu_);
    std::swap(writer_, o.writer_);
    std::swap(writer_done_, o.writer_done_);
    std::swap(readers_, o.readers_);
    return *this;
}

// ------------------------------------------------------------------------------ Ciphertext
Ciphertext::Ciphertext(const SEALContext &context, MemoryPoolHandle) : Ciphertext(context, context.first_parms_id())
{}

Ciphertext::Ciphertext(const SEALContext &context, parms_id_type parms_id, MemoryPoolHandle)
{
    auto cd = context.get_context_data(parms_id);
    if (!cd) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    store_.bind(context);
    parms_id_ = parms_id;
    coeff_modulus_size_ = cd->parms().coeff_modulus().size();
    poly_modulus_degree_ = cd->parms().poly_modulus_degree();
}

void Ciphertext::resize(const SEALContext &context, parms_id_type parms_id, std::size_t size)
{
    auto cd = context.get_context_data(parms_id);
    if (!cd) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    if (size < 2 && size != 0) throw std::invalid_argument("invalid size");
    store_.bind(context);
    parms_id_ = parms_id;
    coeff_modulus_size_ = cd->parms().coeff_modulus().size();
    poly_modulus_degree_ = cd->parms().poly_modulus_degree();
    size_ = size;
    store_.resize_words(size * coeff_modulus_size_ * poly_modulus_degree_);
}

void Ciphertext::resize(const SEALContext &context, std::size_t size)
{
    resize(context, parms_id_ == parms_id_zero ? context.first_parms_id() : parms_id_, size);
}

void Ciphertext::resize(std::size_t size)
{
    if (size < 2 && size != 0) throw std::invalid_argument("invalid size");
    size_ = size;
    store_.resize_words(size * coeff_modulus_size_ * poly_modulus_degree_);
}

bool Ciphertext::is_transparent() const
{
    if (!store_.words() || size_ < 2) return false;
    const std::uint64_t *p = data(1);
    const std::size_t cnt = (size_ - 1) * coeff_modulus_size_ * poly_modulus_degree_;
    return std::all_of(p, p + cnt, [](std::uint64_t x) { return x == 0; });
}

void Plaintext::set_level(const SEALContext &ctx, const parms_id_type &id, std::size_t limbs)
{
    store_.bind(ctx);
    store_.resize_words(limbs * ctx.key_context_data()->parms().poly_modulus_degree(), false);
    parms_id_ = id;
    limbs_ = limbs;
}
} // namespace seal
