// Stand-alone check of csrc/labels.inc.hpp against brute-force restatements written here (tests/test_labels_host_cpu.py builds it
// with the host compiler, under the sanitizers where they exist, and runs it).  Prints "ok <cases>" and returns 0, or the first
// failure and 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>

#include "../redclust.jl_amd/csrc/labels.inc.hpp"

#define REQUIRE(cond)                                                                                       \
    do {                                                                                                    \
        if (!(cond)) { std::printf("FAILED %s (line %d, n = %lld, case %d)\n", #cond, __LINE__, (long long)n, kase); return false; } \
    } while (0)

using Slots = std::vector<std::tuple<int, int64_t, int>>;

// one labelling: compact_labels, dense_ids and cluster_order against sorting the distinct labels
static bool check_labelling(const std::vector<int64_t> &z, int kase)
{
    const int64_t n = (int64_t)z.size();
    std::vector<int64_t> distinct(z);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    const int K = (int)distinct.size();
    Slots want;                                                          // (slot, label, size) in ascending label order
    for (int t = 0; t < K; ++t) want.emplace_back(t, distinct[t], (int)std::count(z.begin(), z.end(), distinct[t]));
    const auto slot_of = [&](int64_t l) { return (int)(std::lower_bound(distinct.begin(), distinct.end(), l) - distinct.begin()); };

    std::vector<int> cnt((size_t)n + 1, 0), id((size_t)n + 1, -1), pos((size_t)n, -1);
    Slots got;
    REQUIRE(compact_labels(z.data(), n, cnt, id, [&](int t, int64_t l, int sz) { got.emplace_back(t, l, sz); }) == K);
    REQUIRE(got == want);
    REQUIRE(std::count(cnt.begin(), cnt.end(), 0) == n + 1);
    std::vector<unsigned short> dense((size_t)n);
    dense_ids(z.data(), n, id, dense.data());
    for (int64_t j = 0; j < n; ++j) REQUIRE(dense[j] == slot_of(z[j]));

    // cluster_order: point j goes to (points of smaller slots) + (earlier points of its slot)
    got.clear();
    std::fill(id.begin(), id.end(), -1);
    std::vector<int> at_of((size_t)n, -1), slot_seen((size_t)n, -1);
    int calls = 0;
    bool in_order = true;
    REQUIRE(cluster_order(z.data(), n, cnt, id, pos, [&](int t, int64_t l, int sz) { got.emplace_back(t, l, sz); },
                          [&](int at, int64_t j, int t) { in_order = in_order && j == calls; ++calls; at_of[j] = at; slot_seen[j] = t; }) == K);
    REQUIRE(got == want && calls == n && in_order);
    REQUIRE(std::count(cnt.begin(), cnt.end(), 0) == n + 1);
    int before = 0;
    for (int t = 0; t < K; ++t) {
        before += std::get<2>(want[t]);
        REQUIRE(pos[t] == before);                                       // one past the slot's last position
    }
    for (int64_t j = 0; j < n; ++j) {
        int at = 0;
        for (int64_t i = 0; i < n; ++i) at += slot_of(z[i]) < slot_of(z[j]) || (z[i] == z[j] && i < j);
        REQUIRE(at_of[j] == at && slot_seen[j] == slot_of(z[j]));
    }
    return true;
}

// find_bad_label on `count` rows of good labels with `bad` written at the given flat positions (none: no offender)
static bool check_bad(std::vector<int64_t> rows, int64_t count, int64_t n, int64_t lo, const std::vector<int64_t> &where, int64_t bad, int kase)
{
    for (int64_t w : where) rows[(size_t)w] = bad;
    int64_t first = -1;                                                   // the restatement: a flat scan
    for (int64_t t = 0; t < count * n && first < 0; ++t)
        if (rows[(size_t)t] < lo || rows[(size_t)t] > n) first = t;
    int64_t row = -7, pos = -7;
    const bool found = find_bad_label(rows.data(), count, n, lo, &row, &pos);
    REQUIRE(found == (first >= 0));
    REQUIRE(found == !where.empty());
    if (found) REQUIRE(row == first / n && pos == first % n);
    else REQUIRE(row == -7 && pos == -7);
    return true;
}

// count_clusters on `count` rows against sorting each row's labels: the counts up to and including the first row above cap, the
// rows behind it untouched
static bool check_counts(const std::vector<int64_t> &rows, int64_t count, int64_t n, int64_t cap, int kase)
{
    std::vector<int> want((size_t)count), got((size_t)count, -7), seen((size_t)n + 1, -1);
    int64_t first = count;
    for (int64_t r = count - 1; r >= 0; --r) {
        std::vector<int64_t> z(rows.begin() + r * n, rows.begin() + (r + 1) * n);
        std::sort(z.begin(), z.end());
        want[(size_t)r] = (int)(std::unique(z.begin(), z.end()) - z.begin());
        if (want[(size_t)r] > cap) first = r;
    }
    REQUIRE(count_clusters(rows.data(), count, n, cap, seen, got.data()) == first);
    for (int64_t r = 0; r < count; ++r) REQUIRE(got[(size_t)r] == (r <= first ? want[(size_t)r] : -7));
    return true;
}

int main()
{
    std::mt19937_64 rng(20240611);
    int cases = 0;
    for (int64_t n : {1, 2, 7, 64}) {
        for (int kase = 0; kase < 300; ++kase, ++cases) {
            std::vector<int64_t> z((size_t)n);
            const int kind = kase % 6;
            const int64_t hi = kind == 3 ? std::max<int64_t>(1, n / 4) : n;  // kind 3: few clusters
            for (int64_t j = 0; j < n; ++j)
                z[j] = kind == 0   ? 1 + (kase / 6) % n                   // all points in one cluster
                       : kind == 1 ? 1 + (j + kase / 6) % n               // all singletons
                       : kind == 2 ? std::max<int64_t>(1, n - (int64_t)(rng() % 2))   // labels from {n − 1, n} only
                                   : 1 + (int64_t)(rng() % (uint64_t)hi);
            if (!check_labelling(z, kase)) return 1;
        }
        // count_clusters: 5 rows of few or many clusters; no row above the cap, every row, or only the rows of many
        for (int kase = 0; kase < 60; ++kase, ++cases) {
            const int64_t count = 5;
            std::vector<int64_t> rows((size_t)(count * n));
            for (int64_t r = 0; r < count; ++r) {
                const int64_t hi = (kase + r) % 3 == 0 ? n : std::max<int64_t>(1, n / 4);
                for (int64_t j = 0; j < n; ++j) rows[(size_t)(r * n + j)] = 1 + (int64_t)(rng() % (uint64_t)hi);
            }
            for (int64_t cap : {n, (int64_t)0, std::max<int64_t>(1, n / 4)})
                if (!check_counts(rows, count, n, cap, kase)) return 1;
        }
        // find_bad_label: 3 rows; the offender first, last, both, twice in between, or absent
        const int64_t count = 3, total = count * n;
        for (int kase = 0; kase < 60; ++kase, ++cases) {
            for (int64_t lo : {0, 1}) {
                std::vector<int64_t> rows((size_t)total);
                for (auto &l : rows) l = lo + (int64_t)(rng() % (uint64_t)(n - lo + 1));   // lo..n, both ends included
                const int64_t bad = kase % 2 ? n + 1 + (int64_t)(rng() % 5) : lo - 1 - (int64_t)(rng() % 5);
                const int64_t a = (int64_t)(rng() % (uint64_t)total), b = (int64_t)(rng() % (uint64_t)total);
                const std::vector<std::vector<int64_t>> wheres = {{}, {0}, {total - 1}, {0, total - 1}, {a}, {a, b}};
                for (const auto &where : wheres)
                    if (!check_bad(rows, count, n, lo, where, bad, kase)) return 1;
            }
        }
    }
    std::printf("ok %d\n", cases);
    return 0;
}
