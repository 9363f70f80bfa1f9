// Host-only boundary run of csrc/wave_input.hpp's wave_check_input, the argument check the three waveform entry points share.
// No device is touched.  Build for the host with the sanitizers and run:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include tools/probe/wave_input_check.hip -o tools/probe/wave_input_check && tools/probe/wave_input_check
#include "../../unispeech_amd/csrc/wave_input.hpp"

static int fails = 0;
static void expect(const char* what, int got, int want) {
  if (got != want) { printf("FAIL %s: %d, expected %d\n", what, got, want); ++fails; }
}

int main() {
  const float sample = 0.f;
  const void* x = &sample;                                  // never read: the check looks at the pointer only
  const int64_t LMAX = INT64_MAX >> 8, L = 16000;           // mfcc / fbank's bound; resample's is INT64_MAX >> 22
  expect("plain", wave_check_input(x, WL_F32, L, 1, L, LMAX), WL_OK);
  expect("null x", wave_check_input(nullptr, WL_F32, L, 1, L, LMAX), WL_EINVAL);
  expect("B = 0", wave_check_input(x, WL_F32, L, 0, L, LMAX), WL_EINVAL);
  expect("B = -1", wave_check_input(x, WL_F32, L, -1, L, LMAX), WL_EINVAL);
  expect("B = 65535", wave_check_input(x, WL_F32, L, 65535, L, LMAX), WL_OK);
  expect("B = 65536", wave_check_input(x, WL_F32, L, 65536, L, LMAX), WL_EINVAL);
  expect("L = 0", wave_check_input(x, WL_F32, 0, 1, 0, LMAX), WL_EINVAL);
  expect("L = 1", wave_check_input(x, WL_F32, 1, 1, 1, LMAX), WL_OK);
  expect("x_stride = L - 1", wave_check_input(x, WL_F32, L - 1, 1, L, LMAX), WL_EINVAL);
  expect("x_stride = L + 1", wave_check_input(x, WL_F32, L + 1, 1, L, LMAX), WL_OK);
  expect("L = max", wave_check_input(x, WL_F32, LMAX, 1, LMAX, LMAX), WL_OK);
  expect("L = max + 1", wave_check_input(x, WL_F32, LMAX + 1, 1, LMAX + 1, LMAX), WL_EINVAL);
  expect("L = max, stride INT64_MAX", wave_check_input(x, WL_I16, INT64_MAX, 65535, LMAX, LMAX), WL_OK);
  expect("resample's max", wave_check_input(x, WL_F32, INT64_MAX >> 22, 1, INT64_MAX >> 22, INT64_MAX >> 22), WL_OK);
  expect("resample's max + 1", wave_check_input(x, WL_F32, LMAX, 1, (INT64_MAX >> 22) + 1, INT64_MAX >> 22), WL_EINVAL);
  const int want[4] = {WL_OK, WL_EINVAL, WL_OK, WL_EINVAL};  // WL_F32, WL_BF16 (not an input), WL_I16, unknown
  for (int dt = 0; dt < 4; ++dt) expect("dtype", wave_check_input(x, dt, L, 1, L, LMAX), want[dt]);
  expect("dtype -1", wave_check_input(x, -1, L, 1, L, LMAX), WL_EINVAL);
  printf(fails ? "wave_check_input: %d FAILED\n" : "wave_check_input: all boundary cases as expected\n", fails);
  return fails ? 1 : 0;
}
