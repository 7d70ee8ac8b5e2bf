// Host utilities of the entry points that own their device memory for one call (most of them take a device number and no
// context): a holder of device buffers, a pair of timing events, the device selection.  Included at the end of
// redclust_hip.hip before every other include (same translation unit: shares fail() and HIPCHK — HIPCHK(nullptr, call)
// reports into the thread's error buffer).  Both holders release on scope exit, so a HIPCHK may return from anywhere.

struct DeviceBuffers {
    std::vector<void *> owned;
    DeviceBuffers() = default;
    DeviceBuffers(const DeviceBuffers &) = delete;
    ~DeviceBuffers() { for (void *q : owned) (void)hipFree(q); }
    // count elements of T into out (null on failure)
    template <typename T> hipError_t alloc(T *&out, size_t count)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e == hipSuccess) owned.push_back(q);
        out = (T *)q;
        return e;
    }
};

struct TimingEvents {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    TimingEvents() = default;
    TimingEvents(const TimingEvents &) = delete;
    ~TimingEvents()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    hipError_t create()
    {
        const hipError_t e = hipEventCreate(&e0);
        return e == hipSuccess ? hipEventCreate(&e1) : e;
    }
};

// The cluster-contiguous order of one labelling z (n labels in 1..n, checked by the caller), shared by predict and the partition
// distances.  The labels are compacted to slots 0..K-1 in ascending label order: slot(t, label, size) is called once per slot,
// in that order.  The points are then counting-sorted by slot: put(at, j, t) is called for every point j, in index order, with
// its position in the sorted order and its slot.  Returns K; afterwards pos[t] is one past slot t's last position.  Scratch of
// the caller's: cnt (n + 1 zeros, left zeroed), slot_of_label (n + 1), pos (n).
template <typename Slot, typename Put>
static int cluster_order(const int64_t *z, int64_t n, std::vector<int> &cnt, std::vector<int> &slot_of_label, std::vector<int> &pos,
                         Slot slot, Put put)
{
    for (int64_t j = 0; j < n; ++j) cnt[(size_t)z[j]]++;
    int K = 0, at = 0;
    for (int64_t l = 1; l <= n; ++l) {
        const int sz = cnt[(size_t)l];
        if (!sz) continue;
        slot_of_label[(size_t)l] = K;
        pos[(size_t)K] = at; at += sz;
        slot(K, l, sz);
        cnt[(size_t)l] = 0;
        ++K;
    }
    for (int64_t j = 0; j < n; ++j) {
        const int t = slot_of_label[(size_t)z[j]];
        put(pos[(size_t)t]++, j, t);
    }
    return K;
}

static int32_t select_device(const char *who, int32_t device)
{
    int ndev = 0;
    HIPCHK(nullptr, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(nullptr, RC_ERR_ARG, "%s: device %d not available (%d visible)", who, device, ndev);
    HIPCHK(nullptr, hipSetDevice(device));
    return RC_OK;
}
