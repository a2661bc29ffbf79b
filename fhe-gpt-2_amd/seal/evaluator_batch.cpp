// evaluator_batch.cpp -- the batched Evaluator entry points (independent operations of one level as
// one engine launch sequence, bit-identical to the calls one by one) and lockstep_execute, which
// runs the calls parked at the merge points of a Lockstep / FiberBatch round through them.
#include "seal_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>

namespace seal
{
// ------------------------------------------------------------------------------ batching switch
namespace
{
std::atomic<bool> g_batched{ true };
std::atomic<std::uint64_t> g_merged_fallbacks{ 0 };
const char *mulsum_fault(const std::vector<const Ciphertext *> &e1, const std::vector<const Ciphertext *> &e2,
                         const std::vector<int> &group, const std::vector<bool> &twice,
                         const std::vector<Ciphertext *> &dst); // (with multiply_sum_rescale below)
} // namespace
void set_batched_launches(bool on)
{
    g_batched.store(on);
}
bool batched_launches()
{
    return g_batched.load();
}

std::uint64_t merged_call_fallbacks(bool reset)
{
    return reset ? g_merged_fallbacks.exchange(0) : g_merged_fallbacks.load();
}

// ------------------------------------------------------------------------------ merged calls
// What each kind of merged call is: run_alone -- one member's call as it would have run without the
// group; run_batch -- the members' entries concatenated (false: the members run alone).
void Evaluator::lockstep_execute(std::vector<LsOp *> &ops) const
{
    auto run_alone = [&](LsOp &o) {
        try
        {
            const bool one = o.in.size() == 1, inplace = one && o.out[0] == o.in[0];
            switch (o.kind)
            {
            case LsOp::ROT:
                if (inplace)
                    rotate_vector_inplace(*o.out[0], o.steps[0], *o.gk);
                else if (one)
                    rotate_vector(*o.in[0], o.steps[0], *o.gk, *o.out[0]);
                else
                    rotate_vectors(o.in, o.steps, *o.gk, o.out);
                break;
            case LsOp::RESC: rescale_to_next_inplace_many(o.out); break;
            case LsOp::RELIN: relinearize_inplace_many(o.out, *o.rk); break;
            case LsOp::MULRE:
                if (inplace)
                    multiply_inplace_reduced_error(*o.out[0], *o.in2[0], *o.rk);
                else
                    multiply_reduced_error(*o.in[0], *o.in2[0], *o.rk, *o.out[0]);
                break;
            case LsOp::ROTSUM: rotate_sum(o.in, o.steps, *o.gk, *o.out[0]); break;
            case LsOp::MULSUM: multiply_sum_rescale(o.in, o.in2, o.steps, o.twice, *o.rk, o.out); break;
            }
        }
        catch (...)
        {
            o.err = std::current_exception();
        }
    };
    auto run_batch = [&]() {
        const LsOp::Kind kind = ops[0]->kind;
        // one group per member, every sum through a temporary; members that cannot share the call
        // (levels, missing keys) run alone
        if (kind == LsOp::ROTSUM) return rotate_sum_merged(ops);
        std::vector<const Ciphertext *> in, in2;
        std::vector<int> steps;
        std::vector<Ciphertext *> dst;
        if (kind == LsOp::MULSUM)
        {
            // the members' sums concatenated; a member whose own call would throw for its arguments
            // makes all run alone
            std::vector<bool> twice;
            for (LsOp *o : ops)
            {
                if (mulsum_fault(o->in, o->in2, o->steps, o->twice, o->out)) return false;
                for (int g : o->steps) steps.push_back(g + (int)dst.size());
                in.insert(in.end(), o->in.begin(), o->in.end());
                in2.insert(in2.end(), o->in2.begin(), o->in2.end());
                twice.insert(twice.end(), o->twice.begin(), o->twice.end());
                dst.insert(dst.end(), o->out.begin(), o->out.end());
            }
            return multiply_sum_merged(in, in2, steps, twice, *ops[0]->rk, dst);
        }
        for (LsOp *o : ops)
        {
            in.insert(in.end(), o->in.begin(), o->in.end());
            in2.insert(in2.end(), o->in2.begin(), o->in2.end());
            steps.insert(steps.end(), o->steps.begin(), o->steps.end());
            dst.insert(dst.end(), o->out.begin(), o->out.end());
        }
        // rescale and relinearize work in place; the others write destinations, so an output that is
        // also an input (in place) or repeated goes through a temporary
        if (kind == LsOp::RESC) return rescale_to_next_inplace_many(dst), true;
        if (kind == LsOp::RELIN) return relinearize_inplace_many(dst, *ops[0]->rk), true;
        std::vector<Ciphertext> tmp(dst.size());
        std::vector<Ciphertext *> out = dst;
        for (std::size_t i = 0; i < dst.size(); i++)
            for (std::size_t j = 0; j < dst.size() && out[i] == dst[i]; j++)
                if ((j < in.size() && dst[i] == in[j]) || (j < in2.size() && dst[i] == in2[j]) ||
                    (j != i && dst[i] == dst[j]))
                    out[i] = &tmp[i];
        if (kind == LsOp::ROT)
            rotate_vectors(in, steps, *ops[0]->gk, out);
        else
            multiply_reduced_error_many(in, in2, *ops[0]->rk, out);
        for (std::size_t i = 0; i < dst.size(); i++)
            if (out[i] != dst[i]) *dst[i] = std::move(tmp[i]);
        return true;
    };
    bool same = ops.size() > 1;
    for (LsOp *o : ops) same = same && o->kind == ops[0]->kind && o->gk == ops[0]->gk && o->rk == ops[0]->rk;
    try
    {
        if (same && run_batch()) return;
    }
    catch (...)
    {
        // The merged call validates every entry before its first launch (rescale / relinearize), or
        // wrote only outputs that are not inputs (rotations, products and sums through temporaries), so the
        // members' operands are unchanged here: each member's call runs again on its own and gets
        // its own result or its own error, as without the group.  Counted (merged_call_fallbacks):
        // a fallback means a merged launch failed, which a healthy run never sees.
        g_merged_fallbacks.fetch_add(1);
    }
    for (LsOp *o : ops) run_alone(*o);
}

void check_destinations(const std::vector<Ciphertext *> &dst, const std::vector<const Ciphertext *> &in,
                        const std::vector<const Ciphertext *> *in2)
{
    for (std::size_t i = 0; i < dst.size(); i++)
    {
        if (!in[i] || (in2 && !(*in2)[i]) || !dst[i]) throw std::invalid_argument("null ciphertext");
        for (std::size_t j = 0; j < dst.size(); j++)
            if ((j != i && dst[i] == dst[j]) || dst[i] == in[j] || (in2 && dst[i] == (*in2)[j]))
                throw std::invalid_argument("destinations must be distinct and must not be inputs");
    }
}

void Evaluator::rotate_vectors(const std::vector<const Ciphertext *> &encrypted, const std::vector<int> &steps,
                               const GaloisKeys &galois_keys, const std::vector<Ciphertext *> &destinations) const
{
    if (merge_point([&] { return LsOp{ LsOp::ROT, encrypted, {}, steps, destinations, &galois_keys }; })) return;
    if (encrypted.size() != steps.size() || encrypted.size() != destinations.size())
        throw std::invalid_argument("encrypted, steps and destinations must have the same size");
    if (!batched_launches())
    {
        for (std::size_t i = 0; i < destinations.size(); i++) rotate_vector(*encrypted[i], steps[i], galois_keys, *destinations[i]);
        return;
    }
    check_destinations(destinations, encrypted, nullptr);
    check_key_parms(context_, galois_keys, "galois_keys");
    EntryTrace tr; // one "rotate" record per entry (the fallbacks below are nested)
    tr.in(encrypted);
    // entries that run batched, grouped by level (chain index)
    std::map<std::size_t, std::vector<std::size_t>> groups;
    std::vector<std::uint32_t> elt(encrypted.size(), 0);
    for (std::size_t i = 0; i < encrypted.size(); i++)
    {
        Level lv = level_of(context_, encrypted[i]->parms_id(), "encrypted");
        if (steps[i] == 0) continue;
        const StepKey k = step_key(lv.n, steps[i], galois_keys);
        if (!k.has_key) continue;
        elt[i] = k.elt;
        groups[lv.L].push_back(i);
    }
    void *s = context_.stream();
    std::vector<bool> done(encrypted.size(), false);
    auto launch = [&](const std::vector<std::size_t> &idx, std::size_t L) {
        std::vector<const std::uint64_t *> in, keys;
        std::vector<std::uint64_t *> out;
        std::vector<std::uint32_t> elts;
        std::vector<int> kls;
        for (std::size_t i : idx)
        {
            check_galois(context_, *encrypted[i], elt[i], galois_keys);
            std::size_t kl = 0;
            keys.push_back(galois_keys.key_for(GaloisKeys::get_index(elt[i]), L, s, kl));
            kls.push_back((int)kl);
            elts.push_back(elt[i]);
        }
        // inputs are read, then destinations re-sized and written (no destination is an input)
        for (std::size_t i : idx) in.push_back(encrypted[i]->store().dev_read(s));
        for (std::size_t i : idx)
        {
            fresh_dest(context_, *encrypted[i], *destinations[i], 2);
            out.push_back(destinations[i]->store().dev_write(s, true));
        }
        chk(mhe_apply_galois_batch(context_.engine(), (int)idx.size(), in.data(), out.data(), elts.data(), keys.data(),
                                   kls.data(), (int)L, s));
        for (std::size_t i : idx) done[i] = true;
    };
    for (auto &g : groups)
    {
        std::vector<std::size_t> idx = g.second;
        if (idx.size() < 2) continue;
        // one call for the level: the engine runs the rotations of an input that appears more than
        // once off one shared ModUp (csrc/hoist.h) and puts the entries of one key side by side in
        // its launches, so they share the key stream (k_ks_row_mac / k_ks_hoist_mac)
        std::stable_sort(idx.begin(), idx.end(), [&](std::size_t a, std::size_t b) { return elt[a] < elt[b]; });
        launch(idx, g.first);
    }
    for (std::size_t i = 0; i < encrypted.size(); i++)
        if (!done[i]) rotate_vector(*encrypted[i], steps[i], galois_keys, *destinations[i]);
    tr.record("rotate", destinations, [&](std::size_t i) { return "\"step\": " + std::to_string(steps[i]); });
}

bool Evaluator::rotate_sum_merged(const std::vector<LsOp *> &ops) const
{
    if (!batched_launches() || trace::enabled() || ops.empty()) return false;
    if (ops[0]->gk->parms_id() != context_.key_parms_id()) return false;
    const parms_id_type &pid = ops[0]->in.empty() || !ops[0]->in[0] ? parms_id_zero : ops[0]->in[0]->parms_id();
    // every rotated term's Galois element, in the order of the launch (group by group)
    std::vector<std::uint32_t> elts;
    for (const LsOp *o : ops)
    {
        if (o->in.empty() || o->in.size() != o->steps.size() || o->gk != ops[0]->gk) return false;
        const std::size_t before = elts.size();
        for (std::size_t i = 0; i < o->in.size(); i++)
        {
            const Ciphertext *c = o->in[i];
            if (!c || c->size() != 2 || !c->is_ntt_form() || c->parms_id() != pid) return false;
            if (o->steps[i] == 0) continue;
            const std::size_t n = c->poly_modulus_degree();
            const std::uint32_t e = mhe_galois_elt_from_step(__builtin_ctzll(n), o->steps[i]);
            if (!e || galois_fault(context_, *c, n, e, *o->gk)) return false;
            elts.push_back(e);
        }
        if (elts.size() == before) return false; // plain adds only
    }
    const Level lv = check_ct(context_, *ops[0]->in[0], "encrypted");
    void *s = context_.stream();
    // every sum into a temporary: a destination may be an input, and keeps its contents when the
    // call throws.  A sum starts from its step-0 terms, if any, and the rotations accumulate.
    std::vector<Ciphertext> res(ops.size());
    auto has_addend = [](const LsOp *o) { return std::find(o->steps.begin(), o->steps.end(), 0) != o->steps.end(); };
    const bool accumulate = has_addend(ops[0]);
    for (const LsOp *o : ops)
        if (has_addend(o) != accumulate) return false; // (members of a group run the same code)
    for (std::size_t g = 0; g < ops.size(); g++)
    {
        const LsOp &o = *ops[g];
        bool started = false;
        for (std::size_t i = 0; i < o.in.size(); i++)
        {
            if (o.steps[i] != 0) continue;
            check_ct(context_, *o.in[i], "encrypted");
            if (!started)
                res[g] = *o.in[i];
            else
            {
                res[g].scale() = o.in[i]->scale(); // add_inplace_reduced_error at equal levels
                add_inplace(res[g], *o.in[i]);
            }
            started = true;
        }
        if (!started) fresh_dest(context_, *o.in[0], res[g], 2);
    }
    std::vector<const std::uint64_t *> in, keys;
    std::vector<int> kls, group;
    std::vector<std::uint64_t *> out;
    in.reserve(elts.size());
    std::size_t term = 0;
    for (std::size_t g = 0; g < ops.size(); g++)
    {
        const LsOp &o = *ops[g];
        for (std::size_t i = 0; i < o.in.size(); i++)
        {
            if (o.steps[i] == 0) continue;
            check_ct(context_, *o.in[i], "encrypted");
            std::size_t kl = 0;
            keys.push_back(o.gk->key_for(GaloisKeys::get_index(elts[term++]), lv.L, s, kl));
            kls.push_back((int)kl);
            group.push_back((int)g);
        }
    }
    for (const LsOp *o : ops)
        for (std::size_t i = 0; i < o->in.size(); i++)
            if (o->steps[i] != 0) in.push_back(o->in[i]->store().dev_read(s));
    for (Ciphertext &r : res) out.push_back(r.store().dev_write(s, !accumulate));
    chk(mhe_rotate_sum(context_.engine(), (int)in.size(), in.data(), elts.data(), keys.data(), kls.data(), group.data(),
                       (int)ops.size(), out.data(), accumulate ? 1 : 0, (int)lv.L, s));
    for (std::size_t g = 0; g < ops.size(); g++)
    {
        res[g].scale() = ops[g]->in.back()->scale(); // what the fold leaves: the last term's scale
        *ops[g]->out[0] = std::move(res[g]);
    }
    return true;
}

void Evaluator::rotate_sum(const std::vector<const Ciphertext *> &encrypted, const std::vector<int> &steps,
                           const GaloisKeys &galois_keys, Ciphertext &destination) const
{
    const auto make = [&] { return LsOp{ LsOp::ROTSUM, encrypted, {}, steps, { &destination }, &galois_keys }; };
    if (merge_point(make)) return;
    if (encrypted.size() != steps.size() || encrypted.empty())
        throw std::invalid_argument("encrypted and steps must have the same, nonzero size");
    for (const Ciphertext *c : encrypted)
        if (!c) throw std::invalid_argument("null ciphertext");
    LsOp op = make();
    std::vector<LsOp *> one{ &op };
    if (rotate_sum_merged(one)) return;
    // one by one: the rotations (batched where rotate_vectors can), then the fold in order
    std::vector<const Ciphertext *> in;
    std::vector<int> st;
    std::vector<Ciphertext> rot(encrypted.size());
    std::vector<Ciphertext *> out;
    for (std::size_t i = 0; i < encrypted.size(); i++)
    {
        if (steps[i] == 0) continue;
        in.push_back(encrypted[i]);
        st.push_back(steps[i]);
        out.push_back(&rot[i]);
    }
    rotate_vectors(in, st, galois_keys, out);
    Ciphertext sum;
    for (std::size_t i = 0; i < encrypted.size(); i++)
    {
        if (i == 0 && steps[i] != 0)
            sum = std::move(rot[i]);
        else if (i == 0)
            sum = *encrypted[i];
        else
            add_inplace_reduced_error(sum, steps[i] != 0 ? rot[i] : *encrypted[i]);
    }
    destination = std::move(sum);
}

void Evaluator::relinearize_inplace_many(const std::vector<Ciphertext *> &encrypted, const RelinKeys &relin_keys) const
{
    if (!batched_launches())
    {
        for (Ciphertext *c : encrypted)
            if (c && c->size() > 2) relinearize_inplace(*c, relin_keys);
        return;
    }
    // relinearize_inplace of every entry; size-3 entries of one level share one batched key switch
    EntryTrace tr; // one "relinearize" record per entry
    tr.in(encrypted);
    check_key_parms(context_, relin_keys, "relin_keys");
    std::map<std::size_t, std::vector<Ciphertext *>> groups;
    for (std::size_t i = 0; i < encrypted.size(); i++)
    {
        Ciphertext *c = encrypted[i];
        if (!c) throw std::invalid_argument("null ciphertext");
        for (std::size_t j = 0; j < i; j++)
            if (encrypted[j] == c) throw std::invalid_argument("entries must be distinct");
        Level lv = check_ct(context_, *c, "encrypted");
        if (!c->is_ntt_form()) throw std::invalid_argument("encrypted must be in NTT form");
        if (c->size() == 3) groups[lv.L].push_back(c);
    }
    void *s = context_.stream();
    // every group's key first (a missing or truncated key throws before any entry is changed: the
    // switches below work in place, and a merged Lockstep / FiberBatch call that throws re-runs its
    // members one by one, lockstep_execute)
    std::map<std::size_t, std::pair<const std::uint64_t *, int>> gkey;
    for (auto &g : groups)
    {
        std::size_t kl = 0;
        const std::uint64_t *k = relin_keys.key_for(RelinKeys::get_index(2), g.first, s, kl);
        gkey[g.first] = { k, (int)kl };
    }
    for (auto &g : groups)
    {
        std::vector<Ciphertext *> &v = g.second;
        if (v.size() < 2) continue; // relinearized one by one below
        const std::size_t L = g.first;
        std::vector<std::uint64_t *> ct;
        std::vector<const std::uint64_t *> target, keys;
        std::vector<int> kls;
        for (Ciphertext *c : v)
        {
            keys.push_back(gkey[L].first);
            kls.push_back(gkey[L].second);
            std::uint64_t *d = c->store().dev_write(s);
            ct.push_back(d);
            target.push_back(d + 2 * L * c->poly_modulus_degree());
        }
        // one engine launch sequence (at most 8 entries, MHE_MAXB) per chunk, and each chunk's entries
        // marked relinearized (size 2) as soon as it is done: the switches work in place, so if a later
        // chunk fails, a member re-run by lockstep_execute finds the finished entries at size 2 and
        // skips them instead of switching them a second time
        constexpr std::size_t kChunk = 8;
        for (std::size_t i0 = 0; i0 < v.size(); i0 += kChunk)
        {
            const int B = (int)std::min(kChunk, v.size() - i0);
            chk(mhe_switch_key_batch(context_.engine(), B, ct.data() + i0, target.data() + i0, keys.data() + i0,
                                     kls.data() + i0, (int)L, s));
            for (int e = 0; e < B; e++) v[i0 + e]->resize(2);
        }
    }
    for (Ciphertext *c : encrypted)
        if (c->size() > 2) relinearize_inplace(*c, relin_keys);
    tr.record("relinearize", encrypted);
}

void Evaluator::multiply_reduced_error_many(const std::vector<const Ciphertext *> &encrypted1,
                                            const std::vector<const Ciphertext *> &encrypted2,
                                            const RelinKeys &relin_keys,
                                            const std::vector<Ciphertext *> &destinations) const
{
    if (encrypted1.size() != encrypted2.size() || encrypted1.size() != destinations.size())
        throw std::invalid_argument("encrypted1, encrypted2 and destinations must have the same size");
    if (!batched_launches())
    {
        for (std::size_t i = 0; i < destinations.size(); i++)
            multiply_reduced_error(*encrypted1[i], *encrypted2[i], relin_keys, *destinations[i]);
        return;
    }
    check_destinations(destinations, encrypted1, &encrypted2);
    EntryTrace tr; // one "mul_re" record per entry
    tr.in(encrypted1);
    tr.in(encrypted2);
    // the products as multiply_reduced_error makes them (size 3), then one batched relinearization
    for (std::size_t i = 0; i < destinations.size(); i++)
    {
        const Ciphertext &a = *encrypted1[i], &b = *encrypted2[i];
        Ciphertext &d = *destinations[i];
        const bool same = a.coeff_modulus_size() == b.coeff_modulus_size() && a.parms_id() == b.parms_id() &&
                          a.size() == 2 && b.size() == 2;
        if (same)
            mulre_product(context_, a, b, d);
        else
        {
            d = a;
            reduced_error_op(d, b, Rmode::mul);
        }
    }
    relinearize_inplace_many(destinations, relin_keys);
    tr.record("mul_re", destinations);
}

// ------------------------------------------------------------------------------ product sums
namespace
{
std::atomic<bool> g_prodsum{ [] {
    const char *e = std::getenv("MHE_PRODSUM");
    return e && e[0] == '1';
}() };

// the first fault in the arguments of a multiply_sum_rescale call (all std::invalid_argument), or
// nullptr: group[] non-decreasing from 0 without a gap, one entry of twice and one destination per
// sum, no null entry, destinations distinct and none of them an input
const char *mulsum_fault(const std::vector<const Ciphertext *> &e1, const std::vector<const Ciphertext *> &e2,
                         const std::vector<int> &group, const std::vector<bool> &twice,
                         const std::vector<Ciphertext *> &dst)
{
    const char *shape = "encrypted1, encrypted2 and group must have the same, nonzero size, and group must number "
                        "the sums of twice and destinations in order";
    const std::size_t terms = e1.size();
    if (terms != e2.size() || terms != group.size() || twice.size() != dst.size() || terms == 0) return shape;
    for (std::size_t i = 0; i < terms; i++)
        if (group[i] != (i ? group[i - 1] : 0) && !(i && group[i] == group[i - 1] + 1)) return shape;
    if ((std::size_t)group.back() + 1 != dst.size()) return shape;
    for (std::size_t i = 0; i < terms; i++)
        if (!e1[i] || !e2[i]) return "null ciphertext";
    for (std::size_t g = 0; g < dst.size(); g++)
    {
        if (!dst[g]) return "null ciphertext";
        for (std::size_t j = 0; j < terms; j++)
            if (dst[g] == e1[j] || dst[g] == e2[j] || (j < dst.size() && j != g && dst[g] == dst[j]))
                return "destinations must be distinct and must not be inputs";
    }
    return nullptr;
}
} // namespace
void set_merged_product_sums(bool on)
{
    g_prodsum.store(on);
}
bool merged_product_sums()
{
    return g_prodsum.load();
}

bool Evaluator::multiply_sum_merged(const std::vector<const Ciphertext *> &encrypted1,
                                    const std::vector<const Ciphertext *> &encrypted2, const std::vector<int> &group,
                                    const std::vector<bool> &twice, const RelinKeys &relin_keys,
                                    const std::vector<Ciphertext *> &destinations) const
{
    if (!batched_launches() || trace::enabled()) return false;
    if (relin_keys.parms_id() != context_.key_parms_id()) return false;
    const std::size_t count = encrypted1.size(), G = destinations.size();
    // the level every product ends at (the lower operand's), one level per sum
    std::vector<std::size_t> level(G, 0), last(G, 0);
    for (std::size_t i = 0; i < count; i++)
    {
        const Ciphertext *a = encrypted1[i], *b = encrypted2[i];
        if (!a || !b || a->size() != 2 || b->size() != 2 || !a->is_ntt_form() || !b->is_ntt_form()) return false;
        const std::size_t L = std::min(a->coeff_modulus_size(), b->coeff_modulus_size()), g = (std::size_t)group[i];
        if (L < 2 || (level[g] && level[g] != L)) return false;
        level[g] = L;
        last[g] = i;
    }
    // the products as multiply_reduced_error_many makes them (size 3)
    std::vector<Ciphertext> prod(count);
    for (std::size_t i = 0; i < count; i++)
    {
        const Ciphertext &a = *encrypted1[i], &b = *encrypted2[i];
        if (a.coeff_modulus_size() == b.coeff_modulus_size() && a.parms_id() == b.parms_id())
            mulre_product(context_, a, b, prod[i]);
        else
        {
            prod[i] = a;
            reduced_error_op(prod[i], b, Rmode::mul);
        }
        if (prod[i].size() != 3 || prod[i].coeff_modulus_size() != level[(std::size_t)group[i]]) return false;
    }
    // a sum carries its last term's scale (add_inplace_reduced_error at equal levels) into the rescale
    std::vector<Rescale> resc;
    resc.reserve(G);
    for (std::size_t g = 0; g < G; g++) resc.push_back(check_rescale(context_, prod[last[g]]));
    void *s = context_.stream();
    std::map<std::size_t, std::vector<std::size_t>> by_level;
    for (std::size_t g = 0; g < G; g++) by_level[level[g]].push_back(g);
    // every level's key before the first launch
    std::map<std::size_t, std::pair<const std::uint64_t *, int>> key;
    for (auto &lv : by_level)
    {
        std::size_t kl = 0;
        const std::uint64_t *k = relin_keys.key_for(RelinKeys::get_index(2), lv.first, s, kl);
        key[lv.first] = { k, (int)kl };
    }
    // every sum into a fresh store, committed to a temporary after its launch and moved to its
    // destination after the last: a call that throws leaves every destination as it was
    std::vector<Ciphertext> res(G);
    std::vector<std::size_t> first(G, count);
    for (std::size_t i = count; i-- > 0;) first[(std::size_t)group[i]] = i;
    for (auto &lv : by_level)
    {
        const std::size_t L = lv.first;
        std::vector<const std::uint64_t *> ct3;
        std::vector<int> grp, tw;
        std::vector<std::uint64_t *> out;
        std::vector<Placed> staged;
        staged.reserve(lv.second.size());
        for (std::size_t g : lv.second)
        {
            for (std::size_t i = first[g]; i <= last[g]; i++)
            {
                ct3.push_back(prod[i].store().dev_read(s));
                grp.push_back((int)tw.size());
            }
            tw.push_back(twice[g] ? 1 : 0);
            staged.emplace_back(context_, Placed::fresh, prod[last[g]], res[g], 2, L - 1);
            out.push_back(staged.back().out(s));
        }
        chk(mhe_relin_sum_rescale(context_.engine(), (int)ct3.size(), ct3.data(), grp.data(), (int)out.size(), tw.data(),
                                  key[L].first, key[L].second, out.data(), (int)L, s));
        for (std::size_t k = 0; k < lv.second.size(); k++)
            staged[k].commit(resc[lv.second[k]].next, resc[lv.second[k]].scale);
    }
    for (std::size_t g = 0; g < G; g++) *destinations[g] = std::move(res[g]);
    return true;
}

void Evaluator::multiply_sum_rescale(const std::vector<const Ciphertext *> &encrypted1,
                                     const std::vector<const Ciphertext *> &encrypted2, const std::vector<int> &group,
                                     const std::vector<bool> &twice, const RelinKeys &relin_keys,
                                     const std::vector<Ciphertext *> &destinations) const
{
    const auto make = [&] {
        LsOp op{ LsOp::MULSUM, encrypted1, encrypted2, group, destinations, nullptr, &relin_keys };
        op.twice = twice;
        return op;
    };
    if (merge_point(make)) return;
    if (const char *f = mulsum_fault(encrypted1, encrypted2, group, twice, destinations)) throw std::invalid_argument(f);
    if (multiply_sum_merged(encrypted1, encrypted2, group, twice, relin_keys, destinations)) return;
    // the sequence itself: the products (relinearizations batched), each sum folded in order and
    // doubled, the rescales batched
    std::vector<Ciphertext> p(encrypted1.size());
    std::vector<Ciphertext *> pp, sums;
    for (Ciphertext &c : p) pp.push_back(&c);
    multiply_reduced_error_many(encrypted1, encrypted2, relin_keys, pp);
    for (std::size_t i = 0; i < p.size(); i++)
    {
        if (i == 0 || group[i] != group[i - 1])
            sums.push_back(&p[i]);
        else
            add_inplace_reduced_error(*sums.back(), p[i]);
        if ((i + 1 == p.size() || group[i + 1] != group[i]) && twice[(std::size_t)group[i]])
            add_inplace_reduced_error(*sums.back(), *sums.back());
    }
    rescale_to_next_inplace_many(sums);
    for (std::size_t g = 0; g < sums.size(); g++) *destinations[g] = std::move(*sums[g]);
}

void Evaluator::rescale_to_next_inplace_many(const std::vector<Ciphertext *> &encrypted) const
{
    if (!batched_launches())
    {
        for (Ciphertext *c : encrypted) rescale_to_next_inplace(*c);
        return;
    }
    // rescale_to_next of every entry; entries of one level and size run as one batched launch
    EntryTrace tr; // one "rescale" record per entry
    tr.in(encrypted);
    // every entry is validated (once) before the first group launches, so a bad entry throws with every
    // ciphertext unchanged (as the first failing one-by-one call would leave the rest)
    struct Entry
    {
        Ciphertext *c;
        Rescale r;
    };
    std::map<std::pair<std::size_t, std::size_t>, std::vector<Entry>> groups;
    for (Ciphertext *c : encrypted)
    {
        if (!c) throw std::invalid_argument("null ciphertext");
        const Rescale r = check_rescale(context_, *c);
        groups[{ r.lv.L, c->size() }].push_back({ c, r });
    }
    // every group's results go to fresh stores first and are committed after the last launch, so
    // a failing group leaves every entry unchanged (a merged Lockstep / FiberBatch call that throws
    // re-runs its members one by one, lockstep_execute)
    void *s = context_.stream();
    std::vector<std::pair<Placed, const Rescale *>> staged;
    staged.reserve(encrypted.size());
    for (auto &g : groups)
    {
        const std::size_t L = g.first.first, size = g.first.second;
        std::vector<const std::uint64_t *> in;
        std::vector<std::uint64_t *> out;
        for (const Entry &e : g.second)
        {
            staged.emplace_back(Placed(context_, Placed::fresh, *e.c, *e.c, size, L - 1), &e.r);
            in.push_back(e.c->store().dev_read(s));
            out.push_back(staged.back().first.out(s));
        }
        chk(mhe_rescale_batch(context_.engine(), (int)g.second.size(), in.data(), out.data(), (int)size, (int)L, s));
    }
    for (auto &e : staged) e.first.commit(e.second->next, e.second->scale);
    tr.record("rescale", encrypted);
}
} // namespace seal
