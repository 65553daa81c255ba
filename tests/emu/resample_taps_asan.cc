// CPU-TEST-ONLY.  The host code that builds the coefficient tables of HIPDEC_SCALE_BILINEAR / _BICUBIC (color.hip: resample_axis_of, resample_taps_of,
// hipdec_resample_taps) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: color.hip compiled for the host against the shim,
// the five library services it calls stubbed here (no table code reaches them).  Built and run by tests/test_resample_sanitizer.py:
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=all -DHIPDEC_HOST_EMU=1 -Itests/emu/shim -Iinclude -Ilibheif_amd/csrc resample_taps_asan.cc -x c++ color.hip
// Every output index of the axes of tests/test_resample_ref.py, each with the exact capacity (a read or write one element past the taps is a heap overflow
// the sanitizer reports) and with capacities below the tap count.
#include "hipdec_internal.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>

namespace hipdec {
int set_error(int code, const char*, ...) { return code; }
hipError_t arena_acquire(void**, size_t, size_t*) { abort(); }
void arena_release(void*, size_t) { abort(); }
hipStream_t default_stream() { abort(); }
int ensure_init() { abort(); }
}  // namespace hipdec

int main()
{
  static const int axes[][2] = {{200, 100}, {200, 37}, {200, 1}, {141, 300}, {93, 93}, {4096, 224}, {17, 224}, {1, 4}, {4096, 1}, {3, 4096}};
  long long taps = 0, calls = 0;
  for (int filter = 16; filter <= 17; filter++)
    for (const auto& ax : axes)
      for (int xx = 0; xx < ax[1]; xx++) {
        int first = -1;
        const int n = hipdec_resample_taps(ax[0], ax[1], filter, xx, &first, nullptr, 0);
        if (n < 1 || first < 0 || first + n > ax[0]) { fprintf(stderr, "axis %d -> %d filter %d sample %d: %d taps from %d\n", ax[0], ax[1], filter, xx, n, first); return 1; }
        const int caps[5] = {n, n - 1, n / 2, 1, 0};
        for (int cap : caps) {
          if (cap < 0) continue;
          std::unique_ptr<int32_t[]> k(new int32_t[cap ? cap : 1]);   // exactly `cap` elements: the sanitizer sees the first write past them
          int f2 = -1;
          if (hipdec_resample_taps(ax[0], ax[1], filter, xx, &f2, cap ? k.get() : nullptr, cap) != n || f2 != first) return 2;
          long long sum = 0;
          for (int i = 0; i < cap; i++) sum += k[i];
          if (cap == n && (sum < (1 << 22) - n || sum > (1 << 22) + n)) { fprintf(stderr, "coefficients of sample %d sum to %lld\n", xx, sum); return 3; }
          calls++;
        }
        taps += n;
      }
  if (hipdec_resample_taps(0, 1, 16, 0, nullptr, nullptr, 0) >= 0 || hipdec_resample_taps(4, 4, 16, 4, nullptr, nullptr, -1) >= 0) return 4;
  printf("RESAMPLE TAPS SANITIZER OK %lld calls %lld taps\n", calls, taps);
  return 0;
}
