// Host-only checks of csrc/conv_f32.hip: every refusal class of iit_conv_f32_ok and three plans against constants
// worked out by hand.  Built with AddressSanitizer on the host half and run on the CPU (tests/test_conv_f32_host.py);
// no kernel is launched and no device memory is touched -- the pointers are made-up addresses the checks only inspect.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

extern "C" {
int iit_conv_f32_ok(int pass, const void* x, const void* w, const void* y, const void* ws, int N, int H, int W,
                    int Cin, int OH, int OW, int Cout, int k, int s, int pad, int tile, int splits);
int iit_conv_f32_plan(int pass, int N, int H, int W, int Cin, int OH, int OW, int Cout, int k, int s, int pad,
                      int tile, int splits, int* out);
}

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
      ++failures;                                                \
    }                                                            \
  } while (0)

struct G {
  int N = 2, H = 6, W = 6, Cin = 4, OH = 3, OW = 3, Cout = 8, k = 3, s = 2, pad = 1;
};

static const void* P(uintptr_t a) { return (const void*)a; }

static int ok(int pass, const G& g, int tile = 0, int splits = 1, uintptr_t x = 0x1000, uintptr_t w = 0x2000,
              uintptr_t y = 0x3000, uintptr_t ws = 0) {
  return iit_conv_f32_ok(pass, P(x), P(w), P(y), P(ws), g.N, g.H, g.W, g.Cin, g.OH, g.OW, g.Cout, g.k, g.s, g.pad, tile,
                         splits);
}

static bool plan_is(int pass, const G& g, int tile, int splits, const int (&want)[6]) {
  int* out = (int*)std::malloc(6 * sizeof(int));  // heap, so that a write past out[5] is an ASan error
  const int rc = iit_conv_f32_plan(pass, g.N, g.H, g.W, g.Cin, g.OH, g.OW, g.Cout, g.k, g.s, g.pad, tile, splits, out);
  bool same = rc == 0;
  for (int i = 0; i < 6 && same; ++i) same = out[i] == want[i];
  if (!same) std::printf("plan: rc %d, got %d %d %d %d %d %d\n", rc, out[0], out[1], out[2], out[3], out[4], out[5]);
  std::free(out);
  return same;
}

int main() {
  const G g;
  for (int pass = 0; pass < 3; ++pass) {
    EXPECT(ok(pass, g) == 1);
    EXPECT(ok(pass, g, 1, 64, 0x1000, 0x2000, 0x3000, 0x4000) == 1);
    // pointers: null, 4-byte misaligned
    EXPECT(ok(pass, g, 0, 1, 0) == 0);
    EXPECT(ok(pass, g, 0, 1, 0x1000, 0) == 0);
    EXPECT(ok(pass, g, 0, 1, 0x1000, 0x2000, 0) == 0);
    EXPECT(ok(pass, g, 0, 1, 0x1002) == 0);
    EXPECT(ok(pass, g, 0, 1, 0x1000, 0x2001) == 0);
    EXPECT(ok(pass, g, 0, 1, 0x1000, 0x2000, 0x3003) == 0);
    EXPECT(ok(pass, g, 0, 1, 0x1004, 0x2008, 0x300c) == 1);  // 4-byte alignment is enough
    // tile and splits
    EXPECT(ok(pass, g, 2) == 0);
    EXPECT(ok(pass, g, -1) == 0);
    EXPECT(ok(pass, g, 0, 0) == 0);
    EXPECT(ok(pass, g, 0, 65, 0x1000, 0x2000, 0x3000, 0x4000) == 0);
    // the split workspace: missing, 16-byte misaligned
    EXPECT(ok(pass, g, 0, 2) == 0);
    EXPECT(ok(pass, g, 0, 2, 0x1000, 0x2000, 0x3000, 0x4004) == 0);
    EXPECT(ok(pass, g, 0, 2, 0x1000, 0x2000, 0x3000, 0x4010) == 1);
    // geometry outside the list
    G b = g; b.k = 8; b.pad = 1; EXPECT(ok(pass, b) == 0);
    b = g; b.k = 0; b.pad = 0; EXPECT(ok(pass, b) == 0);
    b = g; b.s = 3; b.OH = b.OW = 2; EXPECT(ok(pass, b) == 0);
    b = g; b.s = 0; EXPECT(ok(pass, b) == 0);
    b = g; b.pad = 3; b.OH = b.OW = 5; EXPECT(ok(pass, b) == 0);
    b = g; b.pad = -1; b.OH = b.OW = 1; EXPECT(ok(pass, b) == 0);
    b = g; b.N = 0; EXPECT(ok(pass, b) == 0);
    b = g; b.H = 0; EXPECT(ok(pass, b) == 0);
    b = g; b.W = -1; EXPECT(ok(pass, b) == 0);
    b = g; b.Cin = 0; EXPECT(ok(pass, b) == 0);
    b = g; b.Cout = 0; EXPECT(ok(pass, b) == 0);
    b = g; b.H = 1; b.W = 1; b.k = 7; b.pad = 2; b.s = 1; b.OH = b.OW = 1; EXPECT(ok(pass, b) == 0);  // window > image
    // output extents off the formula
    b = g; b.OH = 4; EXPECT(ok(pass, b) == 0);
    b = g; b.OW = 2; EXPECT(ok(pass, b) == 0);
    // extent products beyond int: input, output, weight
    b = g; b.N = 1 << 15; b.H = b.W = 256; b.Cin = 16; b.OH = b.OW = 128; b.Cout = 1; EXPECT(ok(pass, b) == 0);
    b = g; b.N = 1 << 15; b.H = b.W = 256; b.Cin = 1; b.OH = b.OW = 128; b.Cout = 64; EXPECT(ok(pass, b) == 0);
    b = g; b.Cin = 1 << 14; b.Cout = 1 << 14; EXPECT(ok(pass, b) == 0);
    b = g; b.N = 1 << 15; b.H = b.W = 128; b.Cin = 2; b.OH = b.OW = 64; b.Cout = 8; EXPECT(ok(pass, b) == 1);  // 2^30
  }
  // every extreme of the list is accepted
  G e; e.N = 1; e.H = e.W = 1; e.Cin = e.Cout = 1; e.k = 1; e.s = 1; e.pad = 0; e.OH = e.OW = 1;
  EXPECT(ok(0, e) == 1);
  e.k = 7; e.pad = 6; e.s = 2; e.OH = e.OW = 4;  // (1 + 12 - 7) / 2 + 1
  EXPECT(ok(1, e) == 1);

  // plans: {M, N, K, k_per_split, grid.x, vector}
  // forward, the stem at batch 256: 56 x 56 x 3 -> 64, k 7, s 2, pad 3: OH = (56 + 6 - 7) / 2 + 1 = 28;
  // M = 256 * 28 * 28 = 200704, K = 49 * 3 = 147 -> one split of ceil(147 / 32) * 32 = 160; 3136 x 1 tiles of 64
  G a; a.N = 256; a.H = a.W = 56; a.Cin = 3; a.Cout = 64; a.k = 7; a.s = 2; a.pad = 3; a.OH = a.OW = 28;
  EXPECT(plan_is(0, a, 0, 1, {200704, 64, 147, 160, 3136, 0}));
  // input gradient, layer 2's stride-2 conv: 14 x 14 x 64 -> 7 x 7 x 128: M = 256 * 196 = 50176, N = 64,
  // K = 9 * 128 = 1152; tile 1, 2 splits: 576 is a multiple of 16; ceil(50176 / 128) = 392 tiles x 1
  G d; d.N = 256; d.H = d.W = 14; d.Cin = 64; d.Cout = 128; d.k = 3; d.s = 2; d.pad = 1; d.OH = d.OW = 7;
  EXPECT(plan_is(1, d, 1, 2, {50176, 64, 1152, 576, 392, 1}));
  // weight gradient, layer 4's downsample: 4 x 4 x 256 -> 2 x 2 x 512, k 1, s 2: M = 512, N = 256,
  // K = 256 * 4 = 1024; tile 0, 3 splits: ceil(1024 / 3) = 342 -> 11 K-tiles = 352; 8 x 4 tiles
  G wg; wg.N = 256; wg.H = wg.W = 4; wg.Cin = 256; wg.Cout = 512; wg.k = 1; wg.s = 2; wg.pad = 0; wg.OH = wg.OW = 2;
  EXPECT(plan_is(2, wg, 0, 3, {512, 256, 1024, 352, 32, 1}));
  // a refused geometry writes nothing and returns an error
  int out[6] = {-5, -5, -5, -5, -5, -5};
  EXPECT(iit_conv_f32_plan(0, 2, 6, 6, 4, 3, 3, 8, 8, 2, 1, 0, 1, out) != 0 && out[0] == -5 && out[5] == -5);
  EXPECT(iit_conv_f32_plan(0, 2, 6, 6, 4, 3, 3, 8, 3, 2, 1, 0, 1, nullptr) != 0);

  if (failures) {
    std::printf("%d conv_f32 host checks FAILED\n", failures);
    return 1;
  }
  std::printf("conv_f32 host checks passed\n");
  return 0;
}
