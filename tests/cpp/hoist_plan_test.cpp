// The launch plan of a hoisted pass's key MACs (fhe-gpt-2_amd/csrc/hoist_plan.h), on the host: the
// invariants every plan keeps, and the exact plans of a few passes, each derived by hand below from
// the rules of plan_hoist_macs.  Links nothing from the project.  Driven by tests/test_hoist_plan.py.
#include "hoist_plan.h"

#include <cstdio>
#include <string>

static const int MAXB = 8, HOIST_R = 8; // MHE_MAXB (ntt.h), MHE_HOIST_R (hoist.h)

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

// Keys are addresses: key(j) < key(j + 1).
static char g_keys[128];
static const void *key(int j)
{
    return &g_keys[j];
}

// A pass: rotation i of input ent_in[i] by elts[i] under keys[i] / key_limbs[i].
struct Pass
{
    int H = 0;
    std::vector<int> ent_in, key_limbs;
    std::vector<const void *> keys;
    std::vector<uint32_t> elts;
    // input h (appended when new) rotated by 2 * k + 1 under key(k) with kl key limbs
    void add(int h, int k, int kl = 8)
    {
        H = std::max(H, h + 1);
        ent_in.push_back(h);
        keys.push_back(key(k));
        key_limbs.push_back(kl);
        elts.push_back(2 * (uint32_t)k + 1);
    }
    int count() const
    {
        return (int)ent_in.size();
    }
    std::vector<HoistLaunch> plan() const
    {
        return plan_hoist_macs(H, count(), ent_in.data(), keys.data(), key_limbs.data(), elts.data(), MAXB, HOIST_R);
    }
};

static void invariants(const std::string &name, const Pass &p, const std::vector<HoistLaunch> &plan)
{
    std::vector<int> seen(p.count(), 0);
    for (size_t l = 0; l < plan.size(); l++)
    {
        const HoistLaunch &hl = plan[l];
        const std::string at = name + " launch " + std::to_string(l);
        check(at + ": 1 .. MAXB items", !hl.items.empty() && hl.items.size() <= (size_t)MAXB);
        check(at + ": a shared launch has at least 2 items", !hl.shared || hl.items.size() >= 2);
        for (const HoistItem &it : hl.items)
        {
            check(at + ": one rotation count", it.second.size() == hl.items[0].second.size());
            check(at + ": 1 .. HOIST_R rotations", !it.second.empty() && it.second.size() <= (size_t)HOIST_R);
            check(at + ": input in range", it.first >= 0 && it.first < p.H);
            for (size_t r = 0; r < it.second.size(); r++)
            {
                const int i = it.second[r];
                const bool in_range = i >= 0 && i < p.count();
                check(at + ": rotation in range", in_range);
                if (!in_range) continue;
                seen[i]++;
                check(at + ": a rotation of the item's input", p.ent_in[i] == it.first);
                if (r) check(at + ": keys non-decreasing", !(p.keys[i] < p.keys[it.second[r - 1]]));
                if (hl.shared && r < hl.items[0].second.size())
                {
                    const int i0 = hl.items[0].second[r];
                    check(at + ": shared items list equal (key, key_limbs, element)",
                          p.keys[i] == p.keys[i0] && p.key_limbs[i] == p.key_limbs[i0] && p.elts[i] == p.elts[i0]);
                }
            }
        }
    }
    for (int i = 0; i < p.count(); i++) check(name + ": rotation " + std::to_string(i) + " in exactly one item", seen[i] == 1);
}

static std::string show(const std::vector<HoistLaunch> &plan)
{
    std::string s;
    for (const HoistLaunch &hl : plan)
    {
        s += hl.shared ? "S" : "N";
        for (const HoistItem &it : hl.items)
        {
            s += " " + std::to_string(it.first) + ":";
            for (size_t r = 0; r < it.second.size(); r++) s += (r ? "," : "") + std::to_string(it.second[r]);
        }
        s += " | ";
    }
    return s;
}

// the plan of p, checked for the invariants and against `want` (show()'s notation: per launch S(hared)
// or N, then input:rotation,rotation,... per item)
static void expect(const std::string &name, const Pass &p, const std::string &want)
{
    const std::vector<HoistLaunch> plan = p.plan();
    invariants(name, p, plan);
    const std::string got = show(plan);
    check(name + ": plan\n  got  " + got + "\n  want " + want, got == want);
}

static std::string seq(int from, int to, int step = 1)
{
    std::string s;
    for (int i = from; i != to + step; i += step) s += (s.empty() ? "" : ",") + std::to_string(i);
    return s;
}

int main()
{
    {
        // (a) one input, 9 rotations with distinct keys, given in falling key order: rotation i under
        // key(8 - i).  Sorted by key the input's list is 8, 7, .. 0; cut at HOIST_R = 8 it gives the
        // items [8 .. 1] and [0].  Their counts differ, so neither finds a partner for a shared
        // launch.  Left: both, sorted by count (8 before 1); the cut at a change of count makes two
        // launches, the item of 8 first.
        Pass p;
        for (int i = 0; i < 9; i++) p.add(0, 8 - i);
        expect("a", p, "N 0:" + seq(8, 1, -1) + " | N 0:0 | ");
    }
    {
        // (b) three inputs, each rotated under key(2), key(0), key(1) in that order: input h has
        // rotations 3h, 3h + 1, 3h + 2, by key 3h + 1, 3h + 2, 3h.  Items: 0:[1,2,0], 1:[4,5,3],
        // 2:[7,8,6].  From item 0 the search finds items 1 and 2 equal at every position (same key,
        // key_limbs and element): one shared launch of Z = 3, nothing left.
        Pass p;
        for (int h = 0; h < 3; h++)
            for (int k : { 2, 0, 1 }) p.add(h, k);
        expect("b", p, "S 0:1,2,0 1:4,5,3 2:7,8,6 | ");
    }
    {
        // (c) nine inputs rotated alike under key(0), key(1): items h:[2h, 2h + 1].  From item 0 the
        // search stops at MAXB = 8 gathered items (0 .. 7): one shared launch of 8.  Item 8 then
        // searches from 9 on, finds nobody, and stays behind: alone in a non-shared launch.
        Pass p;
        for (int h = 0; h < 9; h++)
            for (int k : { 0, 1 }) p.add(h, k);
        std::string want = "S";
        for (int h = 0; h < 8; h++) want += " " + std::to_string(h) + ":" + seq(2 * h, 2 * h + 1);
        expect("c", p, want + " | N 8:16,17 | ");
    }
    {
        // (d) inputs with 5, 2, 5 and 1 rotations, rotation i under key(i): no key in common.  Items
        // 0:[0..4], 1:[5,6], 2:[7..11], 3:[12]; no two are equal, so no shared launch.  Sorted by
        // count, largest first and stable: inputs 0, 2 (5 each, in input order), 1 (2), 3 (1); cut
        // at every change of count: 5, 5 | 2 | 1.
        Pass p;
        const int counts[4] = { 5, 2, 5, 1 };
        for (int h = 0, i = 0; h < 4; h++)
            for (int r = 0; r < counts[h]; r++, i++) p.add(h, i);
        expect("d", p, "N 0:" + seq(0, 4) + " 2:" + seq(7, 11) + " | N 1:5,6 | N 3:12 | ");
    }
    {
        // (e) the most one pass holds, MAXB inputs with HOIST_R rotations each, rotation i under
        // key(i): 8 items of 8, none equal to another, one count: a single non-shared launch of
        // MAXB items in input order.
        Pass p;
        for (int h = 0; h < MAXB; h++)
            for (int r = 0; r < HOIST_R; r++) p.add(h, h * HOIST_R + r);
        std::string want = "N";
        for (int h = 0; h < MAXB; h++) want += " " + std::to_string(h) + ":" + seq(8 * h, 8 * h + 7);
        expect("e", p, want + " | ");
        // ... and rotated alike (input h's rotation r under key(r)): one shared launch of MAXB items
        Pass q;
        for (int h = 0; h < MAXB; h++)
            for (int r = 0; r < HOIST_R; r++) q.add(h, r);
        want[0] = 'S';
        expect("e alike", q, want + " | ");
    }
    {
        // ties: one input under key(1), key(0), key(1), key(0).  The sort by key is stable, so equal
        // keys keep the order of their rotations: [1, 3, 0, 2].
        Pass p;
        for (int k : { 1, 0, 1, 0 }) p.add(0, k);
        expect("ties", p, "N 0:1,3,0,2 | ");
    }
    {
        // two inputs under the same keys and elements, but input 1's first key with another
        // key_limbs: the lists differ, so no shared launch; both items (one count) in one launch.
        Pass p;
        p.add(0, 0);
        p.add(0, 1);
        p.add(1, 0, 7);
        p.add(1, 1);
        expect("key_limbs", p, "N 0:0,1 1:2,3 | ");
    }
    {
        // an item that found no partner is still offered to later items: inputs 0 and 2 alike (2
        // rotations), input 1 different (2 rotations under other keys).  Shared: 0 and 2; left: 1.
        Pass p;
        p.add(0, 0);
        p.add(0, 1);
        p.add(1, 2);
        p.add(1, 3);
        p.add(2, 0);
        p.add(2, 1);
        expect("skip", p, "S 0:0,1 2:4,5 | N 1:2,3 | ");
    }
    {
        Pass p; // no rotation: no launch
        expect("empty", p, "");
    }
    std::printf("hoist_plan_test: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
