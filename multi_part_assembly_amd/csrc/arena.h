// One bump allocator for every caller-owned workspace (host only).  A workspace's layout is ONE carve function that takes
// its fields from an Arena in order; its size is that same function run on an Arena without a base, which only counts.
#pragma once
#include <cstdint>

namespace mpa {
class Arena {
 public:
  explicit Arena(void* base) : base_(static_cast<char*>(base)) {}
  // `count` elements of T that start on a multiple of `align` bytes from the base and occupy a multiple of `align` bytes
  // (the padding behind a field belongs to it: the total includes the last field's).  nullptr while counting.
  template <class T>
  T* take(int64_t count, int64_t align) {
    const int64_t at = (off_ + align - 1) / align * align;
    off_ = at + (count * (int64_t)sizeof(T) + align - 1) / align * align;
    return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  int64_t bytes() const { return off_; }
  template <class T>
  int64_t elems() const { return (off_ + (int64_t)sizeof(T) - 1) / (int64_t)sizeof(T); }

 private:
  char* base_;
  int64_t off_ = 0;
};
}  // namespace mpa
