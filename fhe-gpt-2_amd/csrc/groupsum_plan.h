// The plan of a grouped sum of key switches (groupsum.h; mhe_rotate_sum, mhe_relin_sum_rescale): which
// entries go into which launch, and which group accumulators each launch writes or adds to.  Host logic
// on integers and pointers only: no HIP, no context, so a plain C++ compiler builds it for
// tests/cpp/groupsum_plan_test.cpp.
#pragma once

#include <algorithm>
#include <numeric>
#include <vector>

// group[] non-decreasing from 0 to groups - 1 without a gap: no group is empty.
static bool check_groups(const int *group, int count, int groups)
{
    for (int i = 0, prev = 0; i < count; prev = group[i++])
        if (group[i] != prev && !(i > 0 && group[i] == prev + 1)) return false;
    return (count ? group[count - 1] + 1 : 0) == groups;
}

// One launch: up to max_b entries, of the Z <= max_b groups they belong to.
struct GroupSumChunk
{
    std::vector<int> entries; // indices into the call's arrays, in launch order
    std::vector<int> zof;     // per entry: its group among the chunk's, 0 .. Z - 1
    std::vector<int> slot;    // per z: the group's slot in the round, group - g0
    std::vector<int> first;   // per z: 1 in the group's first chunk of the round (write, do not add)
    int Z() const { return (int)slot.size(); }
};

// One round: groups g0 .. g0 + G - 1 (G <= max_b), their entries in chunks, then the callers' tail.
struct GroupSumRound
{
    int g0, G;
    std::vector<int> terms; // per slot: the group's entries
    std::vector<GroupSumChunk> chunks;
};

// The rounds of a call, in issue order: max_b groups per round; a round's entries (sorted by keys[],
// stable, when keys is given: a launch's entries of one key share the key stream; else in input order)
// cut into chunks of max_b that cross group boundaries; a chunk's groups numbered z in order of their
// first entry.  group[] as check_groups accepts it.
template <class Key>
static std::vector<GroupSumRound> plan_group_sums(int count, const int *group, int groups, int max_b, const Key *keys)
{
    std::vector<GroupSumRound> plan;
    std::vector<int> order(count);
    std::iota(order.begin(), order.end(), 0);
    for (int g0 = 0, i0 = 0, i1; g0 < groups; g0 += max_b, i0 = i1)
    {
        GroupSumRound r{ g0, std::min(max_b, groups - g0), {}, {} };
        for (i1 = i0; i1 < count && group[i1] < g0 + r.G; i1++) {}
        r.terms.assign(r.G, 0);
        for (int i = i0; i < i1; i++) r.terms[group[i] - g0]++;
        if (keys)
            std::stable_sort(order.begin() + i0, order.begin() + i1, [&](int a, int b) { return keys[a] < keys[b]; });
        std::vector<char> started(r.G, 0); // the round's groups that a chunk has written
        for (int b0 = i0; b0 < i1; b0 += max_b)
        {
            GroupSumChunk ch;
            ch.entries.assign(order.begin() + b0, order.begin() + std::min(i1, b0 + max_b));
            for (int i : ch.entries)
            {
                const int slot = group[i] - g0;
                int z = 0;
                while (z < ch.Z() && ch.slot[z] != slot) z++;
                if (z == ch.Z())
                {
                    ch.slot.push_back(slot);
                    ch.first.push_back(started[slot] ? 0 : 1);
                    started[slot] = 1;
                }
                ch.zof.push_back(z);
            }
            r.chunks.push_back(std::move(ch));
        }
        plan.push_back(std::move(r));
    }
    return plan;
}
