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

static int32_t select_device(const char *who, int32_t device)
{
    int ndev = 0;
    HIPCHK(nullptr, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(nullptr, RC_ERR_ARG, "%s: device %d not available (%d visible)", who, device, ndev);
    HIPCHK(nullptr, hipSetDevice(device));
    return RC_OK;
}
