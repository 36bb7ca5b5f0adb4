// CRS::generate_crs_with_key / set_extraction_key / extract (include/gs_amd.hpp) on the GPU through the C ABI: the key
// that generate_crs_with_key hands out opens commitments to what was committed (group elements themselves, scalars as
// their images), a wrong key and a hiding CRS are refused, and a cleared key opens nothing.
// Input: the case blob of tests/test_gpu_cpp_host.py (u32 curve, type, m, n; then length-prefixed (u64) sections
//   u0 u1 v0 v1 g1 g2 gt X Y ...; a PairingProduct case, the sections after Y are not read).
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
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  uint32_t hdr[4];
  f.read((char*)hdr, sizeof hdr);
  const int curve = (int)hdr[0];
  const uint32_t ty = hdr[1], m = hdr[2], n = hdr[3];
  if (ty != 0) return 2;
  Bytes u0 = section(f), u1 = section(f), v0 = section(f), v1 = section(f), g1 = section(f), g2 = section(f),
        gt = section(f), X = section(f), Y = section(f);
  const G1Affine p1{g1};
  const G2Affine p2{g2};
  auto xvars = split<G1Affine>(X, m);
  auto yvars = split<G2Affine>(Y, n);

  // the same draws give the same CRS, with and without the key
  MixRng ra{0xC0FFEEull}, rb{0xC0FFEEull};
  CRS plain = CRS::generate_crs(p1, p2, ra, curve, 0);
  auto made = CRS::generate_crs_with_key(p1, p2, rb, curve, 0);
  const CRS& crs = made.first;
  const ExtractionKey& key = made.second;
  CHECK(cat(plain.u) == cat(crs.u) && cat(plain.v) == cat(crs.v) && plain.gt_gen.v == crs.gt_gen.v);
  CHECK(ra.s == rb.s);  // four draws each
  CHECK(key.a1.v.size() == 32 && key.a2.v.size() == 32 && !(key.a1 == key.a2));

  MixRng rng{0xFACEull};
  Commit1 cx = batch_commit_G1(xvars, crs, rng);
  Commit2 cy = batch_commit_G2(yvars, crs, rng);
  CHECK(refused([&] { crs.extract(cx.coms); }));  // no key installed yet
  crs.set_extraction_key(key);
  CHECK(cat(crs.extract(cx.coms)) == X);
  CHECK(cat(crs.extract(cy.coms)) == Y);
  CHECK(crs.extract(std::vector<Com1>{}).empty() && crs.extract(std::vector<Com2>{}).empty());

  // scalars come back as their images x * generator
  std::vector<Fr> xs{rng.fr(), rng.fr(), rng.fr()};
  Commit1 sx = batch_commit_scalar_to_B1(xs, crs, rng);
  Commit2 sy = batch_commit_scalar_to_B2(xs, crs, rng);
  Bytes k = cat(xs), img1(xs.size() * crs.ctx->sz[2]), img2(xs.size() * crs.ctx->sz[3]);
  crs.ctx->chk(gs_g1_mul_batch(crs.ctx->c, xs.size(), p1.v.data(), 1, k.data(), img1.data()));
  crs.ctx->chk(gs_g2_mul_batch(crs.ctx->c, xs.size(), p2.v.data(), 1, k.data(), img2.data()));
  CHECK(cat(crs.extract(sx.coms)) == img1);
  CHECK(cat(crs.extract(sy.coms)) == img2);

  // a wrong key is refused and leaves no key behind
  CHECK(refused([&] { crs.set_extraction_key(ExtractionKey{key.a2, key.a1}); }));
  CHECK(refused([&] { crs.extract(cx.coms); }));
  crs.set_extraction_key(key);
  CHECK(cat(crs.extract(cx.coms)) == X);
  crs.clear_extraction_key();
  CHECK(refused([&] { crs.extract(cy.coms); }));

  // a commitment of the wrong size is the reference's kind of panic
  bool threw = false;
  try {
    crs.set_extraction_key(key);
    std::vector<Com1> bad = cx.coms;
    bad[0].v.pop_back();
    crs.extract(bad);
  } catch (const Panic&) {
    threw = true;
  }
  CHECK(threw);

  // the hiding key of the same scalars binds nothing: its key is refused
  {
    Bytes sc;
    MixRng rc{0xC0FFEEull};
    for (int i = 0; i < 4; i++) {
      Fr s = rc.fr();
      sc.insert(sc.end(), s.v.begin(), s.v.end());
    }
    Bytes raw(crs.ctx->sz[5]);
    crs.ctx->chk(gs_crs_generate_hiding(crs.ctx->c, p1.v.data(), p2.v.data(), sc.data(), raw.data()));
    size_t a = crs.ctx->sz[2], b = crs.ctx->sz[3], o = 0;
    auto take = [&](size_t len) {
      Bytes t(raw.begin() + o, raw.begin() + o + len);
      o += len;
      return t;
    };
    std::vector<Com1> hu{{take(2 * a)}, {take(2 * a)}};
    std::vector<Com2> hv{{take(2 * b)}, {take(2 * b)}};
    G1Affine hg1{take(a)};
    G2Affine hg2{take(b)};
    GT hgt{take(crs.ctx->sz[4])};
    CRS hid(hu, hv, hg1, hg2, hgt, curve, 0);
    CHECK(hid.u[0] == crs.u[0] && !(hid.u[1] == crs.u[1]));
    CHECK(refused([&] { hid.set_extraction_key(key); }));
    Commit1 hx = batch_commit_G1(xvars, hid, rng);
    CHECK(refused([&] { hid.extract(hx.coms); }));
  }
  (void)u0, (void)u1, (void)v0, (void)v1, (void)gt;
  std::printf("OK %d\n", checks);
  return 0;
}
