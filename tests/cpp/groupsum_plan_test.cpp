// The launch plan of a grouped sum of key switches (fhe-gpt-2_amd/csrc/groupsum_plan.h), on the host:
// the invariants every plan keeps over a sweep of small cases, the exact plans of the shapes the GPU
// tests use, each derived by hand below from the rules of plan_group_sums, and what check_groups
// accepts.  Links nothing from the project.  Driven by tests/test_groupsum_plan.py.
#include "groupsum_plan.h"

#include <cstdio>
#include <string>

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
static char g_keys[64];
static const void *key(int j)
{
    return &g_keys[j];
}

// group[] of groups with the given sizes, in order
static std::vector<int> groups_of(const std::vector<int> &sizes)
{
    std::vector<int> g;
    for (size_t k = 0; k < sizes.size(); k++) g.insert(g.end(), sizes[k], (int)k);
    return g;
}

static void invariants(const std::string &name, const std::vector<int> &group, int groups, int max_b,
                       const std::vector<const void *> *keys, const std::vector<GroupSumRound> &plan)
{
    const int count = (int)group.size();
    std::vector<int> seen(count, 0), firsts(groups, 0);
    int g_next = 0, terms_sum = 0;
    for (size_t ri = 0; ri < plan.size(); ri++)
    {
        const GroupSumRound &r = plan[ri];
        const std::string at = name + " round " + std::to_string(ri);
        check(at + ": rounds tile the groups", r.g0 == g_next);
        check(at + ": 1 .. max_b groups", r.G >= 1 && r.G <= max_b && r.g0 + r.G <= groups);
        check(at + ": full but for the last", r.G == max_b || r.g0 + r.G == groups);
        g_next = r.g0 + r.G;
        check(at + ": one term count per group", (int)r.terms.size() == r.G);
        std::vector<int> in_round, terms(r.G, 0), began(r.G, 0);
        for (size_t ci = 0; ci < r.chunks.size(); ci++)
        {
            const GroupSumChunk &ch = r.chunks[ci];
            const std::string cat = at + " chunk " + std::to_string(ci);
            const int B = (int)ch.entries.size(), Z = ch.Z();
            check(cat + ": 1 .. max_b entries", B >= 1 && B <= max_b);
            check(cat + ": full but for the round's last", B == max_b || ci + 1 == r.chunks.size());
            check(cat + ": zof per entry, first per z", (int)ch.zof.size() == B && (int)ch.first.size() == Z);
            check(cat + ": 1 .. max_b groups", Z >= 1 && Z <= max_b && Z <= B);
            std::vector<int> used(Z, 0);
            for (int z = 0; z < Z; z++)
            {
                const bool ok = ch.slot[z] >= 0 && ch.slot[z] < r.G;
                check(cat + ": slot in the round", ok);
                if (!ok) continue;
                for (int y = 0; y < z; y++) check(cat + ": slots distinct", ch.slot[y] != ch.slot[z]);
                // first in exactly the earliest chunk that holds the group
                check(cat + ": first[z] is the group's earliest chunk", ch.first[z] == (began[ch.slot[z]] ? 0 : 1));
                firsts[r.g0 + ch.slot[z]] += ch.first[z];
            }
            for (int z = 0; z < Z; z++)
                if (ch.slot[z] >= 0 && ch.slot[z] < r.G) began[ch.slot[z]] = 1;
            for (int e = 0; e < B && (int)ch.zof.size() == B; e++)
            {
                const int i = ch.entries[e], z = ch.zof[e];
                const bool ok = i >= 0 && i < count && z >= 0 && z < Z;
                check(cat + ": entry and its z in range", ok);
                if (!ok) continue;
                seen[i]++;
                used[z]++;
                check(cat + ": the entry's group is in this round", group[i] >= r.g0 && group[i] < r.g0 + r.G);
                check(cat + ": slot == group - g0", ch.slot[z] == group[i] - r.g0);
                // z numbered in order of first appearance
                if (used[z] == 1)
                    for (int y = z + 1; y < Z; y++) check(cat + ": z in order of first entry", used[y] == 0);
                terms[group[i] - r.g0]++;
                in_round.push_back(i);
            }
            for (int z = 0; z < Z; z++) check(cat + ": every z has an entry", used[z] > 0);
        }
        for (int z = 0; z < r.G && (int)r.terms.size() == r.G; z++)
        {
            check(at + ": terms[z] counts the group's entries", r.terms[z] == terms[z] && terms[z] > 0);
            terms_sum += r.terms[z];
        }
        for (size_t k = 1; k < in_round.size(); k++)
        {
            const int a = in_round[k - 1], b = in_round[k];
            if (keys)
                check(at + ": stable key order", (*keys)[a] < (*keys)[b] || ((*keys)[a] == (*keys)[b] && a < b));
            else
                check(at + ": input order", a < b);
        }
    }
    check(name + ": rounds cover the groups", g_next == groups);
    check(name + ": term counts sum to count", terms_sum == count);
    for (int i = 0; i < count; i++) check(name + ": entry " + std::to_string(i) + " in exactly one chunk", seen[i] == 1);
    for (int g = 0; g < groups; g++) check(name + ": group " + std::to_string(g) + " first exactly once", firsts[g] == 1);
}

// per round "R g0+G t=terms,.. :" then per chunk "entries,.. z slot,.. f first,.. zof ..;"
static std::string show(const std::vector<GroupSumRound> &plan)
{
    auto list = [](const std::vector<int> &v) {
        std::string s;
        for (size_t k = 0; k < v.size(); k++) s += (k ? "," : "") + std::to_string(v[k]);
        return s;
    };
    std::string s;
    for (const GroupSumRound &r : plan)
    {
        s += "R " + std::to_string(r.g0) + "+" + std::to_string(r.G) + " t=" + list(r.terms) + " : ";
        for (const GroupSumChunk &ch : r.chunks)
            s += list(ch.entries) + " z " + list(ch.slot) + " f " + list(ch.first) + " zof " + list(ch.zof) + "; ";
    }
    return s;
}

static void expect(const std::string &name, const std::vector<int> &sizes, const std::vector<const void *> *keys,
                   const std::string &want)
{
    const std::vector<int> group = groups_of(sizes);
    const std::vector<GroupSumRound> plan =
        plan_group_sums((int)group.size(), group.data(), (int)sizes.size(), 8, keys ? keys->data() : (const void *const *)nullptr);
    invariants(name, group, (int)sizes.size(), 8, keys, plan);
    const std::string got = show(plan);
    check(name + ": plan\n  got  " + got + "\n  want " + want, got == want);
}

int main()
{
    // ---- the sweep: every plan's invariants.  Group sizes from a small generator (1 .. 10), counts
    // 0 .. 20, max_b 8 and 3, without keys and with keys that repeat and are out of order
    unsigned rnd = 12345;
    auto next = [&]() { return (rnd = rnd * 1103515245u + 12345u) >> 16; };
    for (int count = 0; count <= 20; count++)
        for (int rep = 0; rep < 12; rep++)
        {
            std::vector<int> sizes;
            for (int left = count; left > 0;)
            {
                // rep 0: all ones; rep 1: one group; else random sizes 1 .. 10
                const int s = rep == 0 ? 1 : std::min(left, rep == 1 ? 10 : 1 + (int)(next() % 10));
                sizes.push_back(s);
                left -= s;
            }
            const std::vector<int> group = groups_of(sizes);
            std::vector<const void *> keys(count);
            for (int i = 0; i < count; i++) keys[i] = key((int)(next() % 4));
            for (int max_b : { 8, 3 })
                for (int with_keys = 0; with_keys < 2; with_keys++)
                {
                    const std::string name = "sweep count " + std::to_string(count) + " rep " + std::to_string(rep) + " max_b " +
                                             std::to_string(max_b) + (with_keys ? " keys" : "");
                    check(name + ": check_groups accepts", check_groups(group.data(), count, (int)sizes.size()));
                    invariants(name, group, (int)sizes.size(), max_b, with_keys ? &keys : nullptr,
                               plan_group_sums(count, group.data(), (int)sizes.size(), max_b, with_keys ? keys.data() : (const void *const *)nullptr));
                }
        }

    // ---- exact plans at max_b = 8, without keys (mhe_relin_sum_rescale; mhe_rotate_sum under one key)
    // (3, 1, 5): 9 entries of 3 groups, one round.  Chunk 0 takes entries 0 .. 7: groups 0, 1, 2 in
    // order of appearance (z = slot), all first; zof 0,0,0,1,2,2,2,2.  Chunk 1 is entry 8 alone, of
    // group 2: its only z is slot 2, not first.
    expect("3-1-5", { 3, 1, 5 }, nullptr, "R 0+3 t=3,1,5 : 0,1,2,3,4,5,6,7 z 0,1,2 f 1,1,1 zof 0,0,0,1,2,2,2,2; 8 z 2 f 0 zof 0; ");
    // 8 x 2: 16 entries of 8 groups, one round of two full chunks: groups 0 .. 3, then 4 .. 7 (z from 0
    // again, slots 4 .. 7), every group whole in its chunk and so first there.
    expect("8x2", std::vector<int>(8, 2), nullptr,
           "R 0+8 t=2,2,2,2,2,2,2,2 : 0,1,2,3,4,5,6,7 z 0,1,2,3 f 1,1,1,1 zof 0,0,1,1,2,2,3,3; "
           "8,9,10,11,12,13,14,15 z 4,5,6,7 f 1,1,1,1 zof 0,0,1,1,2,2,3,3; ");
    // 9 x 1: 9 groups make two rounds: groups 0 .. 7 with one chunk of 8 (z = slot), then group 8
    // alone (slot 0 of its round, entry 8).
    expect("9x1", std::vector<int>(9, 1), nullptr,
           "R 0+8 t=1,1,1,1,1,1,1,1 : 0,1,2,3,4,5,6,7 z 0,1,2,3,4,5,6,7 f 1,1,1,1,1,1,1,1 zof 0,1,2,3,4,5,6,7; "
           "R 8+1 t=1 : 8 z 0 f 1 zof 0; ");
    // (9, 8): 17 entries, one round.  Chunk 0: entries 0 .. 7 of group 0.  Chunk 1: entry 8 (group 0,
    // z 0, not first) and 9 .. 15 (group 1, z 1, first).  Chunk 2: entry 16 of group 1, not first.
    expect("9-8", { 9, 8 }, nullptr,
           "R 0+2 t=9,8 : 0,1,2,3,4,5,6,7 z 0 f 1 zof 0,0,0,0,0,0,0,0; "
           "8,9,10,11,12,13,14,15 z 0,1 f 0,1 zof 0,1,1,1,1,1,1,1; 16 z 1 f 0 zof 0; ");
    // one group of 17: chunks of 8, 8 and 1, first only in the first.
    expect("17", { 17 }, nullptr,
           "R 0+1 t=17 : 0,1,2,3,4,5,6,7 z 0 f 1 zof 0,0,0,0,0,0,0,0; "
           "8,9,10,11,12,13,14,15 z 0 f 0 zof 0,0,0,0,0,0,0,0; 16 z 0 f 0 zof 0; ");
    {
        // with keys: (3, 1, 5) again, entry i under key(2 - i % 3): keys 2,1,0,2,1,0,2,1,0.  Sorted by
        // key, stable: key 0 -> 2,5,8; key 1 -> 1,4,7; key 2 -> 0,3,6.  Chunk 0 is the first eight,
        // 2,5,8,1,4,7,0,3: groups in order of appearance 0 (entry 2), 2 (entry 5), 1 (entry 3), so
        // slots 0,2,1 and zof 0,1,1,0,1,1,0,2; all first.  Chunk 1: entry 6 of group 2, not first.
        std::vector<const void *> keys(9);
        for (int i = 0; i < 9; i++) keys[i] = key(2 - i % 3);
        expect("3-1-5 keys", { 3, 1, 5 }, &keys, "R 0+3 t=3,1,5 : 2,5,8,1,4,7,0,3 z 0,2,1 f 1,1,1 zof 0,1,1,0,1,1,0,2; 6 z 2 f 0 zof 0; ");
        // the sort stays inside a round: 9 x 1 with falling keys reverses round 0 only
        for (int i = 0; i < 9; i++) keys[i] = key(8 - i);
        expect("9x1 keys", std::vector<int>(9, 1), &keys,
               "R 0+8 t=1,1,1,1,1,1,1,1 : 7,6,5,4,3,2,1,0 z 7,6,5,4,3,2,1,0 f 1,1,1,1,1,1,1,1 zof 0,1,2,3,4,5,6,7; "
               "R 8+1 t=1 : 8 z 0 f 1 zof 0; ");
    }
    expect("empty", {}, nullptr, "");

    // ---- check_groups: what both entry points accept
    {
        const int ok[] = { 0, 0, 1, 2, 2 }, dec[] = { 0, 1, 0 }, gap[] = { 0, 2 }, no0[] = { 1, 1, 2 }, neg[] = { -1, 0 };
        check("groups: 0,0,1,2,2 of 3", check_groups(ok, 5, 3));
        check("groups: 0,0,1,2,2 of 4 (the last group empty)", !check_groups(ok, 5, 4));
        check("groups: 0,0,1,2,2 of 2 (too few)", !check_groups(ok, 5, 2));
        check("groups: decreasing", !check_groups(dec, 3, 2));
        check("groups: a gap", !check_groups(gap, 2, 3));
        check("groups: group 0 empty", !check_groups(no0, 3, 3));
        check("groups: negative", !check_groups(neg, 2, 1));
        check("groups: a prefix 0,0 of 1", check_groups(ok, 2, 1));
        check("groups: no entry, no group", check_groups(nullptr, 0, 0));
        check("groups: no entry, one group", !check_groups(nullptr, 0, 1));
    }
    std::printf("groupsum_plan_test: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
