// The plan of a hoisted pass's key MACs (rotate.h run_galois_hoisted, step 2): which rotations go
// into which k_ks_hoist_mac / k_ks_hoist_mac_sh launch, and in which order.  Host logic on integers
// and pointers only: no HIP, no context, so a plain C++ compiler builds it for
// tests/cpp/hoist_plan_test.cpp.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

// An item: one input h (index into the pass's inputs) and up to max_r of its rotations (indices into
// the pass's entries), sorted by key.
typedef std::pair<int, std::vector<int>> HoistItem;

// One launch: up to max_b items of one rotation count.  shared: every item lists the same (key,
// key_limbs, element) at every position, so the launch reads each key once (k_ks_hoist_mac_sh).
struct HoistLaunch
{
    bool shared;
    std::vector<HoistItem> items;
};

// The launches of a pass over H inputs and count rotations, rotation i of input ent_in[i] by element
// elts[i] under keys[i] / key_limbs[i], in the order they are issued:
//  - per input, its rotations sorted by key (stable) and cut into items of at most max_r: the items
//    of inputs rotated alike then list the same keys;
//  - items with one (key, key_limbs, element) list gathered, in item order and up to max_b at a time,
//    into shared launches (an item without a partner stays behind);
//  - the items left, sorted by rotation count, largest first (stable), and cut at max_b items or a
//    change of count.
static std::vector<HoistLaunch> plan_hoist_macs(int H, int count, const int *ent_in, const void *const *keys,
                                                const int *key_limbs, const uint32_t *elts, int max_b, int max_r)
{
    std::vector<std::vector<int>> per(H);
    for (int i = 0; i < count; i++) per[ent_in[i]].push_back(i);
    std::vector<HoistItem> items;
    for (int h = 0; h < H; h++)
    {
        std::stable_sort(per[h].begin(), per[h].end(), [&](int a, int b) { return keys[a] < keys[b]; });
        for (size_t r0 = 0; r0 < per[h].size(); r0 += max_r)
            items.emplace_back(h, std::vector<int>(per[h].begin() + r0,
                                                   per[h].begin() + std::min(per[h].size(), r0 + max_r)));
    }
    std::vector<HoistLaunch> plan;
    std::vector<char> done(items.size(), 0);
    for (size_t z0 = 0; z0 < items.size(); z0++)
    {
        if (done[z0]) continue;
        std::vector<size_t> same{ z0 };
        for (size_t z = z0 + 1; z < items.size() && same.size() < (size_t)max_b; z++)
        {
            if (done[z] || items[z].second.size() != items[z0].second.size()) continue;
            bool eq = true;
            for (size_t r = 0; eq && r < items[z].second.size(); r++)
            {
                const int a = items[z].second[r], b = items[z0].second[r];
                eq = keys[a] == keys[b] && key_limbs[a] == key_limbs[b] && elts[a] == elts[b];
            }
            if (eq) same.push_back(z);
        }
        if (same.size() < 2) continue;
        plan.push_back(HoistLaunch{ true, {} });
        for (size_t z : same)
        {
            plan.back().items.push_back(items[z]);
            done[z] = 1;
        }
    }
    std::vector<HoistItem> left;
    for (size_t z = 0; z < items.size(); z++)
        if (!done[z]) left.push_back(items[z]);
    // one rotation count per launch (k_ks_hoist_mac<R>): items ordered by it
    std::stable_sort(left.begin(), left.end(),
                     [](const HoistItem &a, const HoistItem &b) { return a.second.size() > b.second.size(); });
    for (size_t z0 = 0; z0 < left.size();)
    {
        size_t zn = z0 + 1;
        while (zn < left.size() && zn - z0 < (size_t)max_b && left[zn].second.size() == left[z0].second.size()) zn++;
        plan.push_back(HoistLaunch{ false, std::vector<HoistItem>(left.begin() + z0, left.begin() + zn) });
        z0 = zn;
    }
    return plan;
}
