// seal_internal.h -- what the units of libmhe_seal.so share.  Private: not installed, and all of it
// has hidden visibility, so nothing here is exported from the library.
#pragma once
#include "seal/seal.h"

#include "../../include/mhe.h"
#include "trace.h"

#include <exception>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)
namespace seal
{
[[noreturn]] void raise(int rc); // the engine's last error as the exception SEAL throws for it
inline void chk(int rc)
{
    if (rc != MHE_OK) raise(rc);
}

bool are_close(double a, double b);
void require_set(const SEALContext &ctx);
std::shared_ptr<UniformRandomGeneratorFactory> factory_of(const SEALContext &ctx);
std::vector<std::uint64_t> moduli_of(const SEALContext &ctx);

// temporary device buffer on stream s
struct DevBuf
{
    mhe_ctx *eng;
    void *s;
    std::uint64_t *p = nullptr;
    DevBuf(mhe_ctx *e, void *st, std::size_t words) : eng(e), s(st)
    {
        void *q = nullptr;
        chk(mhe_malloc_async(eng, &q, (words ? words : 1) * 8, s));
        p = static_cast<std::uint64_t *>(q);
    }
    ~DevBuf() { (void)mhe_free_async(eng, p, s); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

void sym_encrypt_zero(const SEALContext &ctx, const prng_seed_type &seed, const std::uint64_t *sk, std::size_t limbs,
                      std::uint64_t *c0, std::uint64_t *c1, void *s);

// ------------------------------------------------------------------------------ trace
// One traced operation (trace.h): the input ids are taken at entry, the output id at a normal exit;
// nested operations (depth > 0) and operations that throw leave no record.
template <class F>
class TraceOp
{
public:
    TraceOp(const char *op, F out) : op_(op), out_(out), unc_(std::uncaught_exceptions()) {}
    bool top() const { return sc_.top(); }
    void in(std::initializer_list<std::string> v) { in_.assign(v.begin(), v.end()); }
    std::string extra;
    ~TraceOp()
    {
        if (!sc_.top() || std::uncaught_exceptions() != unc_) return;
        try
        {
            trace::record(op_, in_, out_(), extra);
        }
        catch (...)
        {
        }
    }

private:
    trace::Scope sc_;
    const char *op_;
    F out_;
    std::vector<std::string> in_;
    int unc_;
};
#define TRACE_OP(NAME, OUT, ...)                                                   \
    TraceOp trace_op_(NAME, [&]() -> std::string { return OUT; });             \
    if (trace_op_.top()) trace_op_.in({ __VA_ARGS__ })
#define TRACE_EXTRA(S) \
    if (trace_op_.top()) trace_op_.extra = (S)

// The per-entry records of a batched entry point: in() takes the entries' input ids at entry,
// record() writes one record per entry at a normal exit (the calls it falls back to are nested).
class EntryTrace
{
public:
    template <class P>
    void in(const std::vector<P> &entries) // one more input per entry (a null entry has none)
    {
        if (!sc_.top()) return;
        for (const P &e : entries) in_.push_back(e ? trace::ct(*e) : std::string());
    }
    template <class Extra = std::string (*)(std::size_t)>
    void record(const char *op, const std::vector<Ciphertext *> &out,
                Extra extra = [](std::size_t) { return std::string(); }) const
    {
        for (std::size_t i = 0; sc_.top() && i < out.size(); i++)
        {
            std::vector<std::string> in;
            for (std::size_t k = i; k < in_.size(); k += out.size()) in.push_back(in_[k]);
            trace::record(op, in, trace::ct(*out[i]), extra(i));
        }
    }

private:
    trace::Scope sc_;
    std::vector<std::string> in_; // [input][entry]
};

// ------------------------------------------------------------------------------ argument checks
struct Level
{
    std::size_t L, n;
    double total_bits;
    std::shared_ptr<const SEALContext::ContextData> cd;
};
Level level_of(const SEALContext &ctx, const parms_id_type &id, const char *what);
Level check_ct(const SEALContext &ctx, const Ciphertext &ct, const char *what);
void check_scale(double scale, const Level &lv); // is_scale_within_bounds (evaluator.cpp)
void check_pair(const SEALContext &ctx, const Ciphertext &a, const Ciphertext &b, bool scales);
void check_key_parms(const SEALContext &ctx, const KSwitchKeys &keys, const char *what);
// null entries; a destination that is repeated or also an input (in2 may be null)
void check_destinations(const std::vector<Ciphertext *> &dst, const std::vector<const Ciphertext *> &in,
                        const std::vector<const Ciphertext *> *in2);

// The preconditions of one operation family, in SEAL's order, for the single and the batched forms:
// product and square (the level; the result's scale), Galois after check_ct (galois_fault: the
// text of the first failing one, all std::invalid_argument, or nullptr; n: the ring degree),
// rescale (level, next parms_id, new scale), and the residues of add_const / multiply_const.
Level check_product(const SEALContext &ctx, const Ciphertext &a, const Ciphertext &b, double &new_scale);
Level check_square(const SEALContext &ctx, const Ciphertext &ct, double &new_scale);
const char *galois_fault(const SEALContext &ctx, const Ciphertext &ct, std::size_t n, std::uint32_t elt,
                         const GaloisKeys &keys);
Level check_galois(const SEALContext &ctx, const Ciphertext &ct, std::uint32_t elt, const GaloisKeys &keys);
struct Rescale
{
    Level lv;
    parms_id_type next;
    double scale;
};
Rescale check_rescale(const SEALContext &ctx, const Ciphertext &ct);
std::vector<std::uint64_t> scalar_residues(const SEALContext &ctx, const Ciphertext &ct, double value, Level &lv);
// rotation step (!= 0) -> Galois element -> is its key there; throws "step count too large"
struct StepKey
{
    std::uint32_t elt;
    bool has_key;
};
StepKey step_key(std::size_t n, int step, const GaloisKeys &keys);

// ------------------------------------------------------------------------------ result placement
// destination takes src's level, size, scale and form; its previous contents are not kept (no copy)
void fresh_dest(const SEALContext &ctx, const Ciphertext &src, Ciphertext &dst, std::size_t size);

// Where a launch writes its result: `same` -- dst's own words (in-place forms that keep the shape);
// `fresh` -- a new store that commit() moves into dst after the launch (in-place forms that change
// the shape: dst is intact if the launch throws); `reuse` -- dst's existing allocation, re-shaped
// like src first (out-of-place forms; dst is not an input).
class Placed
{
public:
    enum How { same, fresh, reuse };
    // the result: `size` components of `limbs` limbs
    Placed(const SEALContext &ctx, How how, const Ciphertext &src, Ciphertext &dst, std::size_t size, std::size_t limbs);
    // src's shape: in place when dst is src, else into dst's allocation
    static Placed onto(const SEALContext &ctx, const Ciphertext &src, Ciphertext &dst, std::size_t limbs)
    {
        return Placed(ctx, &src == &dst ? same : reuse, src, dst, src.size(), limbs);
    }
    const std::uint64_t *in(void *s); // src's words (same: the pointer out() returns)
    std::uint64_t *out(void *s);
    void commit(const parms_id_type &id, double scale); // dst is the result: level id, scale, src's form

private:
    const SEALContext &ctx_;
    How how_;
    const Ciphertext &src_;
    Ciphertext &dst_;
    std::size_t size_;
    bool ntt_;
    PolyStore store_;
    std::uint64_t *out_ = nullptr;
};

// the size-3 product of multiply_reduced_error at equal levels (both of size 2), before its
// relinearization: destination (not an input) takes scale encrypted2.scale()^2
void mulre_product(const SEALContext &ctx, const Ciphertext &a, const Ciphertext &b, Ciphertext &destination);

// ------------------------------------------------------------------------------ merge points
// One evaluator call handed to a Lockstep group or a FiberBatch round (lockstep.cpp) and run by
// Evaluator::lockstep_execute (evaluator_batch.cpp).  A new merged operation is a Kind, its cases in
// lockstep_execute and a merge_point() line in its entry point.
struct LsOp
{
    enum Kind
    {
        ROT,
        RESC,
        RELIN,
        MULRE,
        ROTSUM, // in / steps: the terms, out[0]: the sum
        MULSUM  // in / in2: the factors, steps: each product's sum, twice / out: per sum
    } kind = ROT;
    std::vector<const Ciphertext *> in, in2;
    std::vector<int> steps;
    std::vector<Ciphertext *> out;
    const GaloisKeys *gk = nullptr;
    const RelinKeys *rk = nullptr;
    const Evaluator *ev = nullptr;
    std::exception_ptr err{};
    std::vector<bool> twice{};
};

// The merging state is thread-local and private to lockstep.cpp; the other units read it through
// this call only (never inline, so no unit caches a TLS address across swapcontext).  True inside a
// Lockstep group or -- unless group_only -- inside a FiberBatch fiber.
bool merging(bool group_only = false);

template <class Make>
bool Evaluator::merge_point(Make make, bool group_only) const
{
    if (!merging(group_only)) return false;
    LsOp op = make();
    return lockstep_submit(op);
}
} // namespace seal
#pragma GCC visibility pop
