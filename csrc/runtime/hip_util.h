// Shared by the HIP back ends: error check, the owner of a back end's device and pinned
// host allocations, and host-mapped memory as a (host, device) pointer pair.
#pragma once
#include <hip/hip_runtime.h>
#include <stdexcept>
#include <string.h>
#include <string>
#include <vector>

#define HIPCHECK(x)                                                                     \
    do {                                                                                \
        hipError_t e__ = (x);                                                           \
        if (e__ != hipSuccess)                                                          \
            throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e__)); \
    } while (0)

namespace sk {

// Host-mapped memory: the host's pointer and the one kernels use.
template <class T>
struct Mapped {
    T* host = nullptr;
    T* dev = nullptr;
};

// Hands out device and pinned host memory and frees it all in free_all(), at the latest
// when destroyed. `stream`: the encoder's, on which dmalloc() zeroes.
struct HipAllocs {
    hipStream_t stream = nullptr;

    HipAllocs() = default;
    HipAllocs(const HipAllocs&) = delete;
    HipAllocs& operator=(const HipAllocs&) = delete;
    ~HipAllocs() { free_all(); }

    template <class T>
    T* dmalloc(size_t count, bool zero = true) {
        void* p = nullptr;
        HIPCHECK(hipMalloc(&p, count * sizeof(T)));
        dev_.push_back(p);
        if (zero) HIPCHECK(hipMemsetAsync(p, 0, count * sizeof(T), stream));
        return (T*)p;
    }
    template <class T>
    T* hmalloc(size_t count, unsigned flags = hipHostMallocDefault) {
        void* p = nullptr;
        HIPCHECK(hipHostMalloc(&p, count * sizeof(T), flags));
        host_.push_back(p);
        memset(p, 0, count * sizeof(T));
        return (T*)p;
    }
    template <class T>
    Mapped<T> mapped(size_t count, unsigned flags = hipHostMallocDefault) {
        Mapped<T> m;
        m.host = hmalloc<T>(count, flags);
        void* d = nullptr;
        HIPCHECK(hipHostGetDevicePointer(&d, m.host, 0));
        m.dev = (T*)d;
        return m;
    }
    void free_all() {
        for (void* p : dev_) hipFree(p);
        for (void* p : host_) hipHostFree(p);
        dev_.clear();
        host_.clear();
    }

   private:
    std::vector<void*> dev_, host_;
};

}  // namespace sk
