// AddressSanitizer + UndefinedBehaviorSanitizer driver for the two host loops of csrc/points_mul.hip: the per-point body of
// k_points_mul (zkmi_selftest_points_mul_each_host) and the per-chunk body of k_fr_powers (zkmi_selftest_fr_powers_host).
// A stand-alone program: host code only, no GPU, nothing loaded into Python.  scripts/points_mul_asan.sh builds it, makes
// the vectors (the scalars of tests/srs_contribute_model.py, expected points from the Python oracle) and runs it.
//   points_mul_asan_driver VECTORS
// VECTORS: for group 1 then 2: uint64 n | n points (wire) | n scalars (32 B) | n expected points (wire), little-endian.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/zkmi.h"
#include "../include/zkmi_testing.h"

static int fails = 0;
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      fails++;                                                       \
    }                                                                \
  } while (0)

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s VECTORS\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  uint64_t total = 0;
  for (int group = 1; group <= 2; group++) {
    const size_t w = group == 1 ? 96 : 192;
    uint64_t n = 0;
    if (!read_exact(f, &n, 8) || n == 0 || n > (1u << 16)) {
      fprintf(stderr, "bad vector file\n");
      return 2;
    }
    // exactly-sized heap buffers: a read or write one element past either end is an AddressSanitizer report
    std::vector<uint8_t> pts(w * n), sc(32 * n), want(w * n), got(w * n, 0xAB);
    if (!read_exact(f, pts.data(), pts.size()) || !read_exact(f, sc.data(), sc.size()) || !read_exact(f, want.data(), want.size())) {
      fprintf(stderr, "short vector file\n");
      return 2;
    }
    EXPECT(zkmi_selftest_points_mul_each_host(group, pts.data(), sc.data(), n, got.data()) == ZKMI_OK);
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; i++) bad += memcmp(got.data() + w * i, want.data() + w * i, w) != 0;
    EXPECT(bad == 0);
    // one point at a time through buffers of one element
    for (uint64_t i = 0; i < n; i += 7) {
      std::vector<uint8_t> p1(pts.begin() + w * i, pts.begin() + w * (i + 1)), s1(sc.begin() + 32 * i, sc.begin() + 32 * (i + 1)), o1(w);
      EXPECT(zkmi_selftest_points_mul_each_host(group, p1.data(), s1.data(), 1, o1.data()) == ZKMI_OK);
      EXPECT(memcmp(o1.data(), want.data() + w * i, w) == 0);
    }
    printf("group %d: %llu multiplications through the kernel's body, %llu differ from the oracle\n", group, (unsigned long long)n,
           (unsigned long long)bad);
    total += n;
  }
  fclose(f);
  // refusals
  {
    std::vector<uint8_t> p(96, 0), s(32, 0xFF), o(96);
    EXPECT(zkmi_selftest_points_mul_each_host(1, p.data(), s.data(), 1, o.data()) == ZKMI_ERR_NON_CANONICAL);
    EXPECT(zkmi_selftest_points_mul_each_host(3, p.data(), s.data(), 1, o.data()) == ZKMI_ERR_BAD_ARG);
    EXPECT(zkmi_selftest_points_mul_each_host(1, nullptr, s.data(), 1, o.data()) == ZKMI_ERR_BAD_ARG);
  }
  // powers: every range against the single indices it covers, across the chunk a lane walks
  uint32_t chunk = 0, window = 0;
  EXPECT(zkmi_selftest_points_mul_shape(&chunk, &window) == ZKMI_OK && chunk > 1);
  uint8_t c[32] = {0}, q[32] = {0};
  for (int i = 0; i < 31; i++) c[i] = (uint8_t)(37 * i + 11), q[i] = (uint8_t)(101 * i + 3);
  const uint64_t starts[] = {0, 1, chunk - 1, chunk, chunk + 1, chunk / 2 + 1, (1ull << 21) - 2, (1ull << 21) - chunk - 3};
  const uint64_t counts[] = {1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk + 5};
  uint64_t ranges = 0;
  for (uint64_t first : starts)
    for (uint64_t count : counts) {
      std::vector<uint8_t> range(32 * count), one(32);
      EXPECT(zkmi_selftest_fr_powers_host(c, q, first, count, range.data()) == ZKMI_OK);
      for (uint64_t m = 0; m < count; m += (count > 8 ? count / 8 : 1)) {
        EXPECT(zkmi_selftest_fr_powers_host(c, q, first + m, 1, one.data()) == ZKMI_OK);
        EXPECT(memcmp(one.data(), range.data() + 32 * m, 32) == 0);
      }
      ranges++;
    }
  {
    std::vector<uint8_t> o(64);
    EXPECT(zkmi_selftest_fr_powers_host(c, q, (1ull << 40) - 1, 2, o.data()) == ZKMI_ERR_BAD_ARG);
    memset(q, 0xFF, 32);
    EXPECT(zkmi_selftest_fr_powers_host(c, q, 0, 2, o.data()) == ZKMI_ERR_NON_CANONICAL);
    EXPECT(zkmi_selftest_fr_powers_host(c, c, 5, 0, nullptr) == ZKMI_OK);
  }
  printf("powers: %llu ranges against their single indices (chunk %u, window %u)\n", (unsigned long long)ranges, chunk, window);
  printf("%s: %llu multiplications, %d failed expectations\n", fails ? "FAILED" : "ok", (unsigned long long)total, fails);
  return fails ? 1 : 0;
}
