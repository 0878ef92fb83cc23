// The one owner of device memory in the host files behind the C ABI (device_handle.h includes it): DeviceArray<T>, a pointer and
// its capacity in elements, freed by its destructor. Every buffer a handle allocates is a member of this type, so a buffer cannot
// be forgotten when the handle is destroyed, and the scratch of one call is a local of it. No other code of those files calls
// hipMalloc or hipFree. Internal: no kernel file includes it.
#pragma once
#include "error_state.h"

#include <hip/hip_runtime.h>
#include <string>

#define HIP_TRY(call)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return twkSetError((e_ == hipErrorOutOfMemory) ? TWK_ERROR_OUT_OF_MEMORY : TWK_ERROR_HIP,    \
                         std::string(#call) + " failed: " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

template<typename T> struct DeviceElement { static constexpr size_t bytes = sizeof(T); };
template<> struct DeviceElement<void> { static constexpr size_t bytes = 1; }; // an untyped block counts bytes

template<typename T> class DeviceArray
{
public:
  DeviceArray() = default;
  DeviceArray(const DeviceArray&) = delete;
  DeviceArray& operator=(const DeviceArray&) = delete;
  ~DeviceArray() { release(); }

  T* get() const { return pointer_; }
  operator T*() const { return pointer_; }
  size_t capacity() const { return capacity_; }
  bool holds(size_t count) const { return pointer_ != nullptr && count <= capacity_; }

  void release()
  {
    if (pointer_) (void) hipFree(pointer_);
    pointer_ = nullptr; capacity_ = 0;
  }

  // Frees what is held and allocates `count` elements, zeroed on `stream` where asked. `bytes`: what `count` elements take where
  // that is not count x sizeof(T) — pixels of a run-time format, a scratch layout. A failure leaves the array empty (the next
  // ensure allocates again) and is an error of the C ABI: out of memory is TWK_ERROR_OUT_OF_MEMORY, on which a pass is halved.
  int allocate(size_t count, bool zeroed = false, hipStream_t stream = nullptr, size_t bytes = 0)
  {
    release();
    if (bytes == 0) bytes = count * DeviceElement<T>::bytes;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    pointer_ = static_cast<T*>(p);
    if (zeroed) HIP_TRY(hipMemsetAsync(pointer_, 0, bytes, stream));
    capacity_ = count;
    return TWK_SUCCESS;
  }

  // At least `count` elements: grows when it holds fewer, or nothing. Without growth, a compare and no HIP call.
  int ensure(size_t count, bool zeroed = false, hipStream_t stream = nullptr, size_t bytes = 0)
  {
    return holds(count) ? TWK_SUCCESS : allocate(count, zeroed, stream, bytes);
  }

private:
  T* pointer_ = nullptr;
  size_t capacity_ = 0;
};

// Arrays that share one capacity: when any of them is short of `count` or gone, all are released (true) for the caller to allocate
// again, so that the old ones are free before the first new one is asked for
template<typename... Arrays> inline bool regrowTogether(size_t count, Arrays&... arrays)
{
  if ((arrays.holds(count) && ...)) return false;
  (arrays.release(), ...);
  return true;
}
