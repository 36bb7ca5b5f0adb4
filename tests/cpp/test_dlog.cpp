// CRS::dlog_prepare / CRS::extract_scalars (include/gs_amd.hpp) on the GPU through the C ABI: small scalars committed
// under a CRS whose key is known come back themselves, byte for byte, and a scalar outside the range comes back as
// nothing.
// Input: argv[1] the case blob of tests/test_gpu_cpp_host.py (u32 curve, type, m, n; then length-prefixed (u64)
//   sections u0 u1 v0 v1 g1 g2 gt ...; only the generators are read); argv[2..] scalars as 64 hex digits each (the 32
//   bytes of an Fr in the boundary form), the LAST of them outside [0, 2^16), the others inside.
// Exit code 0 and "OK <checks>" on success.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "gs_amd.hpp"

using namespace gs_amd;

static int checks = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                    \
    }                                                                  \
    checks++;                                                          \
  } while (0)

struct MixRng {  // splitmix64; the top limb kept below 2^60 so that every draw is a valid scalar (< r) of both curves
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  Fr fr() {
    uint64_t v[4] = {next(), next(), next(), next() >> 4};
    Fr f;
    f.v.resize(32);
    std::memcpy(f.v.data(), v, 32);
    return f;
  }
};

static Bytes section(std::ifstream& f) {
  uint64_t n = 0;
  f.read((char*)&n, 8);
  Bytes b(n);
  f.read((char*)b.data(), n);
  if (!f) {
    std::fprintf(stderr, "short case file\n");
    std::exit(2);
  }
  return b;
}

static Fr from_hex(const char* h) {
  Fr f;
  f.v.resize(32);
  for (int i = 0; i < 32; i++) {
    unsigned b = 0;
    if (std::sscanf(h + 2 * i, "%2x", &b) != 1) std::exit(2);
    f.v[i] = (uint8_t)b;
  }
  return f;
}

template <class FN> static bool refused(FN fn) {
  try {
    fn();
  } catch (const Panic&) {
    return false;  // a shape panic is not a refusal
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  uint32_t hdr[4];
  f.read((char*)hdr, sizeof hdr);
  const int curve = (int)hdr[0];
  Bytes u0 = section(f), u1 = section(f), v0 = section(f), v1 = section(f), g1 = section(f), g2 = section(f);
  const G1Affine p1{g1};
  const G2Affine p2{g2};
  std::vector<Fr> xs;
  for (int i = 2; i < argc; i++) xs.push_back(from_hex(argv[i]));
  const size_t n = xs.size();

  MixRng ra{0xD106ull};
  auto made = CRS::generate_crs_with_key(p1, p2, ra, curve, 0);
  const CRS& crs = made.first;
  MixRng rng{0xFACEull};
  Commit1 sx = batch_commit_scalar_to_B1(xs, crs, rng);
  Commit2 sy = batch_commit_scalar_to_B2(xs, crs, rng);

  crs.set_extraction_key(made.second);
  CHECK(refused([&] { crs.extract_scalars(sx.coms, 16); }));  // no table yet
  crs.dlog_prepare(1, 6);
  crs.dlog_prepare(2, 6);
  auto a = crs.extract_scalars(sx.coms, 16);
  auto b = crs.extract_scalars(sy.coms, 16);
  CHECK(a.size() == n && b.size() == n);
  for (size_t i = 0; i + 1 < n; i++) {
    CHECK(a[i].has_value() && *a[i] == xs[i]);
    CHECK(b[i].has_value() && *b[i] == xs[i]);
  }
  CHECK(!a[n - 1].has_value() && !b[n - 1].has_value());  // outside the range: nothing, not a wrong value
  CHECK(crs.extract_scalars(std::vector<Com1>{}, 16).empty() && crs.extract_scalars(std::vector<Com2>{}, 16).empty());
  CHECK(refused([&] { crs.extract_scalars(sx.coms, 6 + 26); }));  // more than 2^24 giant steps
  CHECK(refused([&] { crs.dlog_prepare(1, 1); }));
  crs.clear_extraction_key();
  CHECK(refused([&] { crs.extract_scalars(sx.coms, 16); }));
  (void)u0, (void)u1, (void)v0, (void)v1;
  std::printf("OK %d\n", checks);
  return 0;
}
