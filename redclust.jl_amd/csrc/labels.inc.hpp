// Host-only helpers for label matrices (rows of n labels, row-major), shared by the point-estimate entry points.  Plain C++17: no
// HIP, no error reporting, no globals — redclust_hip.hip includes it ahead of hostutil.inc.hip, whose check_label_rows turns
// find_bad_label into the library's error, and tests/labels_host.cpp includes it on its own.  Nothing here allocates: the
// scratch vectors are the caller's, sized once per call.
#include <cstdint>
#include <vector>

// The first label outside lo..n in row-major order (lo = 1 for samples and labellings, 0 where 0 means "unallocated"): true,
// with its 0-based row and position; false if there is none.
static inline bool find_bad_label(const int64_t *rows, int64_t count, int64_t n, int64_t lo, int64_t *row, int64_t *pos)
{
    for (int64_t r = 0; r < count; ++r)
        for (int64_t j = 0; j < n; ++j) {
            const int64_t l = rows[(size_t)r * n + j];
            if (l < lo || l > n) { *row = r; *pos = j; return true; }
        }
    return false;
}

// K[r] = the number of distinct labels of row r, for `count` rows of n labels in 1..n (checked by the caller), up to and
// including the first row with more than cap: returns that row, or count if there is none.  seen: n + 1 scratch, all -1.
static inline int64_t count_clusters(const int64_t *rows, int64_t count, int64_t n, int64_t cap, std::vector<int> &seen, int *K)
{
    for (int64_t r = 0; r < count; ++r) {
        const int64_t *z = rows + (size_t)r * n;
        int k = 0;
        for (int64_t j = 0; j < n; ++j)
            if (seen[(size_t)z[j]] != (int)r) { seen[(size_t)z[j]] = (int)r; ++k; }
        K[r] = k;
        if (k > cap) return r;
    }
    return count;
}

// One labelling z (n labels in 1..n, checked by the caller) compacted to slots 0..K-1 in ascending label order: id[label] is
// the slot, and slot(t, label, size) is called once per slot, in that order.  Returns K.  cnt: n + 1 zeros, left zeroed;
// id: n + 1 scratch.
template <typename Slot>
static int compact_labels(const int64_t *z, int64_t n, std::vector<int> &cnt, std::vector<int> &id, Slot slot)
{
    for (int64_t j = 0; j < n; ++j) cnt[(size_t)z[j]]++;
    int K = 0;
    for (int64_t l = 1; l <= n; ++l) {
        const int sz = cnt[(size_t)l];
        if (!sz) continue;
        id[(size_t)l] = K;
        slot(K, l, sz);
        cnt[(size_t)l] = 0;
        ++K;
    }
    return K;
}

// the dense ids of z's points after compact_labels filled id
static inline void dense_ids(const int64_t *z, int64_t n, const std::vector<int> &id, unsigned short *out)
{
    for (int64_t j = 0; j < n; ++j) out[j] = (unsigned short)id[(size_t)z[j]];
}

// The cluster-contiguous order of one labelling z, shared by predict and the partition distances.  The labels are compacted as
// by compact_labels (slot(t, label, size) once per slot).  The points are then counting-sorted by slot: put(at, j, t) is called
// for every point j, in index order, with its position in the sorted order and its slot.  Returns K; afterwards pos[t] is one
// past slot t's last position.  Scratch of the caller's: cnt (n + 1 zeros, left zeroed), slot_of_label (n + 1), pos (n).
template <typename Slot, typename Put>
static int cluster_order(const int64_t *z, int64_t n, std::vector<int> &cnt, std::vector<int> &slot_of_label, std::vector<int> &pos,
                         Slot slot, Put put)
{
    int at = 0;
    const int K = compact_labels(z, n, cnt, slot_of_label, [&](int t, int64_t l, int sz) {
        pos[(size_t)t] = at; at += sz;
        slot(t, l, sz);
    });
    for (int64_t j = 0; j < n; ++j) {
        const int t = slot_of_label[(size_t)z[j]];
        put(pos[(size_t)t]++, j, t);
    }
    return K;
}
