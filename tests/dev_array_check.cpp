// Host check of DevArr<T> (csrc/mempool.h): the byte count an allocation asks the pool for, and the element type of what the array
// hands out.  No HIP call is made: only constant expressions and types are looked at, so nothing of the runtime is linked.
#include <type_traits>
#include <utility>
#include "../global-lvba_amd/csrc/mempool.h"

using lvba::DevArr;

namespace {
struct Rec { double a[3]; int32_t n; }; // 32 bytes with its padding
template <class T> constexpr bool typed()
{
    return std::is_same<decltype(std::declval<DevArr<T> &>().release()), T *>::value &&
           std::is_same<decltype(std::declval<DevArr<T> &>().operator T *()), T *>::value &&
           std::is_convertible<DevArr<T> &, T *>::value && std::is_convertible<const DevArr<T> &, const T *>::value &&
           !std::is_copy_constructible<DevArr<T>>::value && !std::is_copy_assignable<DevArr<T>>::value;
}
static_assert(typed<uint32_t>() && typed<float4>() && typed<Rec>(), "release() and the pointer conversion have the element type");
static_assert(!std::is_convertible<DevArr<int32_t> &, float *>::value && !std::is_convertible<DevArr<uint64_t> &, uint32_t *>::value,
              "an array does not pass for one of another element type");
static_assert(sizeof(float4) == 16 && sizeof(Rec) == 32, "the element sizes this check assumes");
static_assert(DevArr<uint32_t>::bytes_for(1000) == 4000 && DevArr<double>::bytes_for(10 * 77) == 80 * 77, "scalar elements");
static_assert(DevArr<float4>::bytes_for(3) == 48 && DevArr<Rec>::bytes_for(5) == 160, "vector and struct elements");
static_assert(DevArr<uint8_t>::bytes_for(0) == 8 && DevArr<float4>::bytes_for(0) == 8 && DevArr<Rec>::bytes_for(0) == 8,
              "zero elements give the 8-byte minimum");
static_assert(DevArr<uint8_t>::bytes_for(1) == 1 && DevArr<uint8_t>::bytes(0) == 0 && DevArr<int64_t>::bytes(7) == 56, "bytes()");
} // namespace

// what alloc(n) asks the pool for, for the test to hold against its own arithmetic (counts past 2^32 bytes included)
extern "C" unsigned long long dev_array_bytes_for(int kind, unsigned long long n)
{
    return kind == 0 ? DevArr<uint8_t>::bytes_for(n) : kind == 1 ? DevArr<double>::bytes_for(n) : kind == 2 ? DevArr<float4>::bytes_for(n)
                                                                                                  : DevArr<Rec>::bytes_for(n);
}
