// lockstep.cpp -- Lockstep (threads) and FiberBatch (fibers on one thread): evaluator calls parked at
// their merge points run as one merged call per round (Evaluator::lockstep_execute).  The merging
// state is thread-local and private to this unit: see merging() and Evaluator::lockstep_submit.
#include "lockstep_core.h"
#include "seal_internal.h"

#include <atomic>
#include <cstdint>
#include <functional>

#include <csignal>
#include <sys/mman.h>
#include <ucontext.h>
#include <unistd.h>

namespace seal
{
namespace
{
thread_local Lockstep::Impl *tl_ls = nullptr;        // the calling thread's group, while merging
thread_local Lockstep::Impl *tl_ls_member = nullptr; // the group the thread is a member of
thread_local int tl_ls_direct = 0;            // > 0 inside a round's execution: calls run directly
thread_local FiberBatch::Impl *tl_fb = nullptr; // the FiberBatch running on this thread
bool fiber_merging(); // inside a FiberBatch fiber (defined with FiberBatch::Impl)
struct LsDirect
{
    LsDirect() { ++tl_ls_direct; }
    ~LsDirect() { --tl_ls_direct; }
};
} // namespace

// ------------------------------------------------------------------------------ Lockstep
struct Lockstep::Impl
{
    detail::LockstepCore<LsOp> core;
    explicit Impl(std::size_t m) : core(m) {}
    // a round's merged call, run by the member that completes the round (lockstep_core.h)
    static void execute(std::vector<LsOp *> &batch)
    {
        LsDirect d;
        batch[0]->ev->lockstep_execute(batch);
    }
};

// ------------------------------------------------------------------------------ FiberBatch
// Guard pages of the live fiber stacks, lock-free so a signal handler may read them.
static constexpr int kGuardSlots = 4096;
static std::atomic<std::uintptr_t> g_guards[kGuardSlots];
static void guard_list(void *page, bool add)
{
    const std::uintptr_t a = reinterpret_cast<std::uintptr_t>(page);
    for (auto &slot : g_guards)
    {
        std::uintptr_t want = add ? 0 : a;
        if (slot.compare_exchange_strong(want, add ? a : 0)) return;
    }
}

bool fiber_stack_guard(const void *addr)
{
    const std::uintptr_t x = reinterpret_cast<std::uintptr_t>(addr), page = (std::uintptr_t)sysconf(_SC_PAGESIZE);
    for (const auto &slot : g_guards)
    {
        const std::uintptr_t g = slot.load(std::memory_order_relaxed);
        if (g && x >= g && x < g + page) return true;
    }
    return false;
}

struct FiberBatch::Impl
{
    // A fiber's stack: mmap'ed, with a PROT_NONE guard page below it (stacks grow down), so an
    // overflow faults at a known address instead of silently corrupting a neighbouring heap block.
    // Live guard pages are listed in g_guards for fiber_stack_guard (a fault handler's question).
    struct Stack
    {
        void *base = nullptr; // guard page + usable bytes
        std::size_t bytes = 0;
        Stack() = default;
        Stack(const Stack &) = delete;
        Stack &operator=(const Stack &) = delete;
        Stack(Stack &&o) noexcept : base(o.base), bytes(o.bytes) { o.base = nullptr; }
        ~Stack()
        {
            if (!base) return;
            guard_list(base, false);
            munmap(base, bytes);
        }
        void alloc(std::size_t usable)
        {
            const std::size_t page = (std::size_t)sysconf(_SC_PAGESIZE);
            usable = (usable + page - 1) / page * page;
            bytes = usable + page;
            base = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_STACK, -1, 0);
            if (base == MAP_FAILED)
            {
                base = nullptr;
                throw std::runtime_error("FiberBatch: stack allocation failed");
            }
            if (mprotect(base, page, PROT_NONE) != 0) throw std::runtime_error("FiberBatch: guard page failed");
            guard_list(base, true);
        }
        char *sp() const { return static_cast<char *>(base) + (bytes - usable()); }
        std::size_t usable() const { return bytes - (std::size_t)sysconf(_SC_PAGESIZE); }
    };
    struct Fiber
    {
        ucontext_t ctx{};
        Stack stack;
        std::size_t idx = 0;
        bool done = false, blocked = false;
        std::exception_ptr err;
    };
    ucontext_t sched{};
    std::vector<Fiber> fibers;
    Fiber *current = nullptr;
    std::vector<LsOp *> pending;
    // elementwise engine launches parked by the fibers (mhe_set_launch_hook): one per fiber per round
    std::vector<std::pair<mhe_ctx *, mhe_launch *>> launches;
    std::size_t launch_rounds = 0, launches_merged = 0;
    const std::function<void(std::size_t)> *work = nullptr;
    std::size_t rounds = 0, merged = 0;

    // makecontext passes int arguments: the group pointer in two halves
    static void entry(unsigned lo, unsigned hi)
    {
        Impl *g = reinterpret_cast<Impl *>(((std::uintptr_t)hi << 32) | (std::uintptr_t)lo);
        Fiber *f = g->current;
        try
        {
            (*g->work)(f->idx);
        }
        catch (...)
        {
            f->err = std::current_exception();
        }
        f->done = true; // returns to uc_link = the scheduler
    }
    // fiber i's context: its own stack, entry(), back to the scheduler at the end
    __attribute__((noinline)) void init(std::size_t i, std::size_t stack_bytes)
    {
        Fiber &f = fibers[i];
        f.idx = i;
        f.stack.alloc(stack_bytes);
        if (getcontext(&f.ctx) != 0) throw std::runtime_error("FiberBatch: getcontext failed");
        f.ctx.uc_stack.ss_sp = f.stack.sp();
        f.ctx.uc_stack.ss_size = f.stack.usable();
        f.ctx.uc_link = &sched;
        const std::uintptr_t self = reinterpret_cast<std::uintptr_t>(this);
        makecontext(&f.ctx, reinterpret_cast<void (*)()>(&Impl::entry), 2, (unsigned)(self & 0xFFFFFFFFu),
                    (unsigned)(self >> 32));
    }
    // the calling fiber's merge point: park `op` for the round and yield to the scheduler
    void submit(LsOp &op)
    {
        Fiber *f = current;
        pending.push_back(&op);
        f->blocked = true;
        swapcontext(&f->ctx, &sched);
    }
    // the engine's launch hook: inside a fiber the launch is parked for the round (the same-numbered
    // elementwise launches of the fibers run as one batched launch); elsewhere it runs now
    static void launch_hook(mhe_ctx *ctx, mhe_launch *l, void *user)
    {
        Impl *g = static_cast<Impl *>(user);
        if (!g->current || tl_ls_direct > 0)
        {
            mhe_launch *one[1] = { l };
            mhe_launch_run(ctx, one, 1);
            return;
        }
        Fiber *f = g->current;
        g->launches.push_back({ ctx, l });
        f->blocked = true;
        swapcontext(&f->ctx, &g->sched);
    }
    // one round's parked launches, grouped by context (mhe_launch_run batches equal shapes)
    void run_launches()
    {
        while (!launches.empty())
        {
            mhe_ctx *ctx = launches.front().first;
            std::vector<mhe_launch *> ls;
            std::vector<std::pair<mhe_ctx *, mhe_launch *>> rest;
            for (auto &p : launches) (p.first == ctx ? (void)ls.push_back(p.second) : rest.push_back(p));
            mhe_launch_run(ctx, ls.data(), (int)ls.size());
            launch_rounds++;
            if (ls.size() > 1) launches_merged += ls.size();
            launches.swap(rest);
        }
    }
};

namespace
{
thread_local std::size_t tl_fb_rounds = 0, tl_fb_merged = 0;
bool fiber_merging()
{
    return tl_fb && tl_fb->current;
}
} // namespace

void FiberBatch::run(std::size_t count, const std::function<void(std::size_t)> &work, std::size_t stack_bytes)
{
    if (tl_fb) throw std::logic_error("FiberBatch::run: already inside a fiber batch");
    Impl g;
    g.work = &work;
    g.fibers.resize(count);
    for (std::size_t i = 0; i < count; i++) g.init(i, stack_bytes);
    // an alternate signal stack for this thread (if it has none), so a handler installed with
    // SA_ONSTACK can still run -- and report -- when a fiber overflows into its guard page
    struct AltStack
    {
        std::vector<char> mem;
        bool set = false;
        AltStack()
        {
            stack_t cur{};
            if (sigaltstack(nullptr, &cur) == 0 && (cur.ss_flags & SS_DISABLE))
            {
                mem.resize(64 * 1024);
                stack_t st{};
                st.ss_sp = mem.data();
                st.ss_size = mem.size();
                set = sigaltstack(&st, nullptr) == 0;
            }
        }
        ~AltStack()
        {
            if (!set) return;
            stack_t st{};
            st.ss_flags = SS_DISABLE;
            (void)sigaltstack(&st, nullptr);
        }
    } alt;
    tl_fb = &g;
    mhe_set_launch_hook(&Impl::launch_hook, &g);
    struct Reset
    {
        ~Reset()
        {
            mhe_set_launch_hook(nullptr, nullptr);
            tl_fb = nullptr;
        }
    } reset;
    for (;;)
    {
        // every runnable fiber runs to its next merge point (or its end)
        bool ran = false;
        for (auto &f : g.fibers)
            if (!f.done && !f.blocked)
            {
                ran = true;
                g.current = &f;
                swapcontext(&g.sched, &f.ctx);
                g.current = nullptr;
            }
        if (!g.pending.empty() || !g.launches.empty())
        {
            // one round: the parked elementwise launches as batched launches, the parked evaluator
            // calls as one merged call (lockstep_execute), then every parked fiber resumes with its
            // result or its own error (the fibers' data are independent, so the order is free)
            g.run_launches();
            if (!g.pending.empty())
            {
                std::vector<LsOp *> batch;
                batch.swap(g.pending);
                {
                    LsDirect d;
                    batch[0]->ev->lockstep_execute(batch);
                }
                g.rounds++;
                if (batch.size() > 1) g.merged += batch.size();
            }
            for (auto &f : g.fibers) f.blocked = false;
            continue;
        }
        if (!ran) break; // every fiber finished
    }
    tl_fb_rounds = g.rounds + g.launch_rounds;
    tl_fb_merged = g.merged + g.launches_merged;
    for (auto &f : g.fibers)
        if (f.err) std::rethrow_exception(f.err);
}

long FiberBatch::current()
{
    return (tl_fb && tl_fb->current) ? (long)tl_fb->current->idx : -1;
}

std::size_t FiberBatch::last_rounds()
{
    return tl_fb_rounds;
}

std::size_t FiberBatch::last_merged()
{
    return tl_fb_merged;
}

Lockstep::Lockstep(std::size_t members) : impl_(std::make_unique<Impl>(members)) {}
Lockstep::~Lockstep() = default;
std::size_t Lockstep::rounds() const
{
    return impl_->core.rounds();
}
std::size_t Lockstep::merged_calls() const
{
    return impl_->core.merged();
}

Lockstep::Member::Member(Lockstep &group, bool active) : g_(group)
{
    tl_ls_member = group.impl_.get();
    tl_ls = active ? tl_ls_member : nullptr;
}

Lockstep::Active::Active() : saved_(tl_ls) { tl_ls = tl_ls_member; }
Lockstep::Active::~Active() { tl_ls = saved_; }

Lockstep::Member::~Member()
{
    tl_ls = nullptr;
    tl_ls_member = nullptr;
    g_.impl_->core.leave(Impl::execute);
}

bool Evaluator::lockstep_submit(LsOp &op) const
{
    if (tl_ls_direct > 0 || trace::enabled()) return false;
    if (fiber_merging())
    {
        op.ev = this;
        tl_fb->submit(op);
        if (op.err) std::rethrow_exception(op.err);
        return true;
    }
    Lockstep::Impl *g = tl_ls;
    if (!g) return false;
    op.ev = this;
    g->core.submit(&op, Lockstep::Impl::execute);
    if (op.err) std::rethrow_exception(op.err);
    return true;
}

bool merging(bool group_only)
{
    return tl_ls || (!group_only && fiber_merging());
}
} // namespace seal
