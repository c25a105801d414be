// What the host-only drivers of this directory share: the failure counter, fake device pointers, raw array I/O and `main`'s dispatch.
// tests/control_harness.py builds every driver with -fsanitize=address,undefined, -ffp-contract=off and -Wall -Werror and runs it
// directly:
//   DRIVER MODE          one of the driver's checking modes (validate, status, corrupt): one line per failure, then "K failure(s)";
//                        exit status = K (a sanitizer report ends the program with a non-zero status of its own)
//   DRIVER run IN OUT    the driver's computation on the arrays of IN, results to OUT (layouts: the driver's head comment)
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../stove_amd/csrc/validate.h"

inline int failures = 0;
// a validation result: 0 where `want` is 0, else exactly hipErrorInvalidValue
inline void expect(const char* what, int got, int want) {
  if ((got != 0) != (want != 0) || (want != 0 && got != stove_validate::kStoveInvalidValue)) {
    std::printf("FAIL %s: got %d, want %d\n", what, got, want);
    ++failures;
  }
}
inline void check(const char* what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++failures;
  }
}
// "Device" pointers are fake, suitably aligned addresses: a dereference is a sanitizer report
template <typename T>
T* dev(uintptr_t k) { return reinterpret_cast<T*>(uintptr_t(0x7000000000ull) + k * 4096); }   // never mapped

template <typename T>
bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
bool write_v(std::FILE* f, const std::vector<T>& v) {
  return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

struct DriverMode {
  const char* name;
  void (*fn)();
};
inline int driver_main(int argc, char** argv, std::initializer_list<DriverMode> modes, int (*run)(const char*, const char*) = nullptr) {
  for (const DriverMode& m : modes)
    if (argc == 2 && std::strcmp(argv[1], m.name) == 0) {
      m.fn();
      std::printf("%d failure(s)\n", failures);
      return failures;
    }
  if (run != nullptr && argc == 4 && std::strcmp(argv[1], "run") == 0) return run(argv[2], argv[3]);
  std::fprintf(stderr, "usage: %s MODE%s; MODE one of", argv[0], run != nullptr ? " | run IN OUT" : "");
  for (const DriverMode& m : modes) std::fprintf(stderr, " %s", m.name);
  std::fprintf(stderr, "\n");
  return 2;
}
