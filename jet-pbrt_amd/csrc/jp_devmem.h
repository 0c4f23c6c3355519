// jet-pbrt_amd/csrc/jp_devmem.h -- who owns device memory: the only file of this directory that calls hipMalloc / hipFree / hipHostMalloc / hipHostFree.
// DevBuf owns one device allocation (move-only), PinnedBuf one pinned host allocation (neither copied nor moved); both are grow-only and free in their destructor, so a context,
// a builder's result or a call's scratch releases its memory by going out of scope.  Every byte a DevBuf holds is counted in one process-wide
// counter (jp_device_bytes_in_use), so the tests assert that nothing leaks.  Host only; included by jp_kernels.hip before jp_lbvh.h.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <utility>

static std::atomic<long long> g_device_bytes{ 0 };

class DevBuf
{
	void* p_ = nullptr; size_t cap_ = 0;
public:
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
	~DevBuf() { reset(); }
	void reset() { if (p_) { hipFree(p_); g_device_bytes -= (long long)cap_; } p_ = nullptr; cap_ = 0; }
	// grow-only: nothing happens when the capacity suffices; otherwise the old allocation goes first (the contents are not kept) and a failure
	// leaves the buffer empty with zero capacity
	hipError_t reserve(size_t bytes)
	{
		if (bytes <= cap_) return hipSuccess;
		reset();
		const hipError_t e = hipMalloc(&p_, bytes);
		if (e != hipSuccess) { p_ = nullptr; return e; }
		cap_ = bytes; g_device_bytes += (long long)bytes;
		return hipSuccess;
	}
	template <class T> T* get() const { return (T*)p_; }
	size_t bytes() const { return cap_; }
	explicit operator bool() const { return p_ != nullptr; }
};

// reserve and hand out the typed pointer (null after a failure); reserve16: at least 16 bytes, so that an empty table still has an address
template <class T> static inline hipError_t reserve(DevBuf& b, T*& p, size_t bytes) { const hipError_t e = b.reserve(bytes); p = b.get<T>(); return e; }

template <class T> static inline hipError_t reserve16(DevBuf& b, T*& p, size_t bytes) { return reserve(b, p, std::max<size_t>(bytes, 16)); }

// allocate (at least 16 bytes) and copy up (blocking)
static inline hipError_t upload(DevBuf& b, const void* src, size_t bytes)
{
	const hipError_t e = b.reserve(std::max<size_t>(bytes, 16));
	return e != hipSuccess || bytes == 0 ? e : hipMemcpy(b.get<void>(), src, bytes, hipMemcpyHostToDevice);
}

// pinned staging memory of the host: reserve may fail, the caller then copies through pageable memory
class PinnedBuf
{
	void* p_ = nullptr; size_t cap_ = 0;
public:
	PinnedBuf() = default;
	PinnedBuf(const PinnedBuf&) = delete;
	PinnedBuf& operator=(const PinnedBuf&) = delete;
	~PinnedBuf() { reset(); }
	void reset() { if (p_) hipHostFree(p_); p_ = nullptr; cap_ = 0; }
	hipError_t reserve(size_t bytes)
	{
		if (bytes <= cap_) return hipSuccess;
		reset();
		const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
		if (e != hipSuccess) { p_ = nullptr; return e; }
		cap_ = bytes;
		return hipSuccess;
	}
	template <class T> T* get() const { return (T*)p_; }
	size_t bytes() const { return cap_; }
};
