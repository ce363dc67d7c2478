// rt::SkyChain (raytracedggx_amd/csrc/rt_sky_chain.h) on its own: the host's argument for leaving still and settled sky alone, driven
// through scripted frame sequences, every returned decision checked against an expectation written out here with the sentence of the
// header that justifies it.  A stand-alone program, built with AddressSanitizer and UBSan by tests/test_sky_chain_host.py and run as a
// child process.  Nothing of HIP is included.
//
// The scripts are the event lists of tests/test_gpu_static_sky.py and tests/test_gpu_settled_sky.py (a whole frame of 320 x 180, the strip
// of rows 37-150), plus what a GPU test cannot reach: the stale-history guard on its own, and the epoch's wrap.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../raytracedggx_amd/csrc/rt_sky_chain.h"

namespace rt {
struct SkyChainProbe {      // (the header's one friend)
  static uint32_t& tssWrites(SkyChain& c, uint32_t parity) { return c.tssWrites_[parity]; }
};
}  // namespace rt
using rt::SkyBreak;
using rt::SkyChain;

static int g_failed = 0, g_checked = 0;
static void expect(const char* script, const char* step, const char* what, long got, long want, const char* why) {
  ++g_checked;
  if (got == want) return;
  if (g_failed++ < 40) std::printf("FAILED %s / %s: %s is %ld, expected %ld -- %s\n", script, step, what, got, want, why);
}

// The constants the launchers hand to prevRunThreshold (rtggx_context.h RT_SKY_PREV_RUN = RT_SETS + 2, RT_SKY_RUN_CAP)
static const uint32_t PREV_RUN = 6u, RUN_CAP = 255u;
static const int g_streams[2] = {0, 0};

// What the launchers do around the chain: the frame counter, the history parity, the rows of each pass (rtggx_context.h passRows).
struct Sim {
  SkyChain chain;
  uint32_t frame = 0, parity = 0, W = 320, H = 180, contextW = 320, rowBegin = 0, rowEnd = 180, rate = 1, sliceShift = 0;
  bool adaptive = true, diffuse = false, fuse = false;
  const void* stream = &g_streams[0];
  float camera[20];
  Sim() { for (int k = 0; k < 20; ++k) camera[k] = 0.25f * (float)(k + 1); }
  void rows(uint32_t apron, uint32_t& b, uint32_t& e) const {
    b = rowBegin > apron ? rowBegin - apron : 0u; e = rowEnd + apron < H ? rowEnd + apron : H;
    if (rowEnd <= rowBegin) b = e = 0u;
  }
  bool whole() const { return rowBegin == 0u && rowEnd == H && W == contextW; }
  uint32_t gen() {      // launchRayTrace
    SkyChain::GenFacts now;
    rows(18u, now.rows[0], now.rows[1]);
    now.frame = frame; now.rate = rate; now.sliceShift = sliceShift; now.tilesX = (W + 15u) / 16u; now.tilesY = (now.rows[1] - now.rows[0] + 15u) / 16u;
    now.adaptive = adaptive; now.stream = stream; std::memcpy(now.camera, camera, sizeof camera);
    return chain.rayGeneration(now);
  }
  struct Denoise { bool v, words, skip; };
  bool vPass() {
    SkyChain::VFacts now; uint32_t g1;
    rows(18u, now.gbufferRow0, g1); rows(2u, now.rows[0], now.rows[1]);
    now.frame = frame; now.fltRflNull = !diffuse;
    return chain.reflectionV(now);
  }
  Denoise denoise() {      // launchDenoise
    parity ^= 1u;
    Denoise d; d.v = vPass();
    SkyChain::TemporalFacts now; uint32_t g1;
    rows(18u, now.gbufferRow0, g1); rows(1u, now.rows[0], now.rows[1]);
    now.frame = frame; now.parity = parity; now.width = W; now.fused = fuse; now.whole = whole();
    const SkyChain::TemporalDecision t = chain.temporal(now);
    d.words = t.keepsWords; d.skip = t.maySkip;
    if (fuse) chain.backBufferWrittenElsewhere();
    return d;
  }
  bool tone(bool fromTss = true) {      // launchToneMap
    SkyChain::ToneMapFacts now;
    rows(0u, now.rows[0], now.rows[1]);
    now.frame = frame; now.parity = parity; now.fromTss = fromTss; now.whole = whole();
    return chain.toneMap(now);
  }
  struct Frame { uint32_t epoch; bool v, words, skip, tm; };
  Frame next() {      // an ordinary frame: the fused path has no tone map of its own
    ++frame;
    Frame f; f.epoch = gen();
    const Denoise d = denoise(); f.v = d.v; f.words = d.words; f.skip = d.skip;
    f.tm = fuse ? false : tone();
    return f;
  }
};

// One frame's expectations: the four decisions, each with the sentence of rt_sky_chain.h it follows from.
struct Want { bool v; const char* vWhy; bool words; const char* wordsWhy; bool skip; const char* skipWhy; bool tm; const char* tmWhy; };
static void check(const char* script, const char* step, const Sim::Frame& got, uint32_t epoch, const char* epochWhy, const Want& w) {
  expect(script, step, "the epoch", got.epoch, epoch, epochWhy);
  expect(script, step, "reflectionV", got.v, w.v, w.vWhy);
  expect(script, step, "temporal keepsWords", got.words, w.words, w.wordsWhy);
  expect(script, step, "temporal maySkip", got.skip, w.skip, w.skipWhy);
  expect(script, step, "toneMap", got.tm, w.tm, w.tmWhy);
}
static const char* const SAME_FACTS = "the epoch is bumped when this ray generation differs from the one before it: it does not";
// the frame of an event that starts a new epoch: no pass may skip, no words are kept
static const Want NEW_EPOCH = {
  false, "reflectionV: the previous reflection V pass ... had ray generation's results of its own frame under the same epoch",
  false, "temporal: under a NEW epoch it stores none and needs none",
  false, "temporal: it may leave blocks alone when, BESIDES [keeping words] ...",
  false, "toneMap: this frame's temporal pass kept words"};
// the frame after it (and the second frame of a context)
static const Want SECOND = {
  true, "reflectionV: what it would store there is what the PREVIOUS reflection V pass stored, into the same image",
  true, "temporal: it keeps them on whole frames of the two-kernel path ... when the pass before it ran under the same epoch",
  false, "temporal: the temporal pass before this one ... kept words",
  true, "toneMap: this frame's temporal pass kept words ... the tone map before this one was the previous frame's, under the same epoch"};
// from the third frame on
static const Want STEADY = {
  true, SECOND.vWhy, true, SECOND.wordsWhy,
  true, "temporal: the temporal pass before this one was the previous frame's, kept words, over the same rows, and wrote the other history image",
  true, SECOND.tmWhy};

// "Steady state": identical facts every frame.  Every later script starts from the state this one reaches.
static uint32_t steady(Sim& s, const char* script) {
  check(script, "frame 1", s.next(), 2u, "rayGeneration: the very first one has none before it", NEW_EPOCH);
  check(script, "frame 2", s.next(), 2u, SAME_FACTS, SECOND);
  for (int k = 3; k <= 8; ++k) check(script, "frames 3-8", s.next(), 2u, SAME_FACTS, STEADY);
  return 2u;
}
// After an event that must bump the epoch ONCE before or in the next ray generation: a new epoch and no decision in the event's frame, then
// recovery exactly as in the steady state.
static uint32_t recover(Sim& s, const char* script, uint32_t epochBefore, const char* why) {
  const uint32_t e = (epochBefore + 1u) & 0xFFFFFFu;
  check(script, "the event's frame", s.next(), e, why, NEW_EPOCH);
  check(script, "one frame later", s.next(), e, SAME_FACTS, SECOND);
  check(script, "two frames later", s.next(), e, SAME_FACTS, STEADY);
  check(script, "three frames later", s.next(), e, SAME_FACTS, STEADY);
  return e;
}

static void scriptEpochEvents() {
  Sim s; uint32_t e = steady(s, "steady state");
  expect("steady state", "threshold", "prevRunThreshold", s.chain.prevRunThreshold(PREV_RUN, RUN_CAP), PREV_RUN, "the run from which ray generation leaves a tile alone: RT_SKY_PREV_RUN");
  expect("steady state", "grid", "genTilesX", s.chain.genTilesX(), 20, "the tile grid of the most recent ray generation"); expect("steady state", "grid", "genTilesY", s.chain.genTilesY(), 12, "the tile grid of the most recent ray generation");
  expect("steady state", "reason", "lastBreak", (long)s.chain.lastBreak(), (long)SkyBreak::Generation, "Generation: this ray generation differs from the one before it");

  for (int k = 0; k < 20; k += 19) {      // one camera float changed in its last bit: the first of ProjToWorld, the last of EyePt
    uint32_t bits; std::memcpy(&bits, &s.camera[k], 4); bits ^= 1u; std::memcpy(&s.camera[k], &bits, 4);
    e = recover(s, "camera, one bit", e, "rayGeneration: the camera -- rg.ProjToWorld, rg.EyePt, compared bit for bit");
  }
  s.stream = &g_streams[1];
  e = recover(s, "another stream", e, "rayGeneration: the stream -- the previous set's words are ordered before this kernel by stream order only");
  s.rate = 4u; e = recover(s, "rate 4", e, "rayGeneration: the bins -- ray rate");
  s.rate = 1u; e = recover(s, "rate 1 again", e, "rayGeneration: the bins -- ray rate");
  s.adaptive = false; e = recover(s, "adaptive off", e, "rayGeneration: the bins -- adaptive split on / off");
  s.adaptive = true; e = recover(s, "adaptive on", e, "rayGeneration: the bins -- adaptive split on / off");
  s.sliceShift = 1u; e = recover(s, "another slice shift", e, "rayGeneration: the bins -- slice shift");
  s.sliceShift = 0u; e = recover(s, "slice shift 0 again", e, "rayGeneration: the bins -- slice shift");

  // every reason an entry point ends the runs for, between two frames: ray generation then finds nothing changed and bumps no further
  static const struct { SkyBreak why; const char* name; } reasons[] = {
    {SkyBreak::Environment, "breakRuns(Environment)"}, {SkyBreak::Upload, "breakRuns(Upload)"}, {SkyBreak::Strip, "breakRuns(Strip)"}, {SkyBreak::TraceRays, "breakRuns(TraceRays)"},
    {SkyBreak::SetBuffers, "breakRuns(SetBuffers)"}, {SkyBreak::TileWordsSwitch, "breakRuns(TileWordsSwitch)"}, {SkyBreak::FeatureSwitch, "breakRuns(FeatureSwitch)"}};
  for (const auto& r : reasons) {
    s.chain.breakRuns(r.why);
    expect(r.name, "reason", "lastBreak", (long)s.chain.lastBreak(), (long)r.why, "the most recent one is kept for a debugger");
    e = recover(s, r.name, e, "breakRuns: bumped whenever something a sky tile's outputs depend on changes");
  }
  // ... and between the denoiser and the tone map (test_gpu_settled_sky.py: an upload into the history image or the back buffer)
  { ++s.frame;
    expect("upload before the tone map", "ray generation", "the epoch", s.gen(), e, SAME_FACTS);
    const Sim::Denoise d = s.denoise();
    expect("upload before the tone map", "denoise", "reflectionV", d.v, true, STEADY.vWhy); expect("upload before the tone map", "denoise", "temporal maySkip", d.skip, true, STEADY.skipWhy);
    s.chain.breakRuns(SkyBreak::Upload);
    expect("upload before the tone map", "tone map", "toneMap", s.tone(), false, "toneMap: this frame's temporal pass kept words ... under the epoch that is still current");
    e = recover(s, "upload before the tone map", e, "breakRuns: the epoch the upload left; the next ray generation does not differ and bumps no further"); }
}

static void scriptRows() {
  Sim s; uint32_t e = steady(s, "rows: steady state");
  // the strip of the GPU tests: other rows end the runs by ray generation's own comparison; a strip keeps no words
  s.rowBegin = 37u; s.rowEnd = 150u;
  { uint32_t b, x;
    s.rows(18u, b, x); expect("strip", "rows", "G-buffer rows", (long)b * 1000 + x, 19168, "passRows: +-18"); s.rows(2u, b, x); expect("strip", "rows", "V rows", (long)b * 1000 + x, 35152, "passRows: +-2");
    s.rows(1u, b, x); expect("strip", "rows", "temporal rows", (long)b * 1000 + x, 36151, "passRows: +-1"); s.rows(0u, b, x); expect("strip", "rows", "final rows", (long)b * 1000 + x, 37150, "passRows: the strip"); }
  static const Want STRIP = {true, SECOND.vWhy, false, "temporal: it keeps them on whole frames (no strip: no histReach, no peers, no apron rows)", false, NEW_EPOCH.skipWhy, false, NEW_EPOCH.tmWhy};
  ++e; check("strip", "the event's frame", s.next(), e, "rayGeneration: the rows -- another strip: tiles count from the pass's first row", NEW_EPOCH);
  for (int k = 0; k < 4; ++k) check("strip", "still frames", s.next(), e, SAME_FACTS, STRIP);
  s.rowBegin = 0u; s.rowEnd = 180u;
  e = recover(s, "whole frame again", e, "rayGeneration: the rows -- another strip");
  // a frame narrower than six tiles never keeps words
  Sim n; n.W = n.contextW = 80u;
  static const Want NARROW = {true, SECOND.vWhy, false, "temporal: at least six tiles across (temporalKernel's loads)", false, NEW_EPOCH.skipWhy, false, NEW_EPOCH.tmWhy};
  check("width below 96", "frame 1", n.next(), 2u, "rayGeneration: the very first one has none before it", NEW_EPOCH);
  for (int k = 0; k < 4; ++k) check("width below 96", "later frames", n.next(), 2u, SAME_FACTS, NARROW);
  // a frame of another size than the context's is no whole frame
  Sim o; o.contextW = 640u;
  check("not the context's size", "frame 1", o.next(), 2u, "rayGeneration: the very first one has none before it", NEW_EPOCH);
  for (int k = 0; k < 3; ++k) check("not the context's size", "later frames", o.next(), 2u, SAME_FACTS, STRIP);
}

// Chains that break without the epoch moving by an entry point's doing.
static void scriptBrokenChains() {
  { Sim s; const uint32_t e = steady(s, "visibility only: steady state");      // a frame with a visibility pass only: the frame number advances by two between ray generations
    ++s.frame;
    recover(s, "a frame with a visibility pass only", e, "rayGeneration: the frame before was not a ray generation's: a set in the ring went by without one"); }
  { Sim s; const uint32_t e = steady(s, "no denoiser: steady state");      // a frame without the denoiser
    ++s.frame;
    expect("a frame without the denoiser", "that frame", "the epoch", s.gen(), e, SAME_FACTS);
    expect("a frame without the denoiser", "that frame", "toneMap", s.tone(), false, "toneMap: THIS frame's temporal pass kept words (the record is the frame before's)");
    static const Want AFTER = {
      false, "reflectionV: the previous reflection V pass was this frame's or the frame before's (a frame without rtggx_denoise leaves FilteredOut1 a frame old)",
      true, "temporal: the first pass after anything else that breaks the chain -- a fused pass, a frame without the denoiser -- stores `epoch | 0` everywhere",
      false, "temporal: the temporal pass before this one was the previous frame's",
      true, "toneMap: the tone map before this one was the previous frame's ... and read the OTHER history image as it still is (no temporal pass has written it since)"};
    check("a frame without the denoiser", "one frame later", s.next(), e, SAME_FACTS, AFTER);
    check("a frame without the denoiser", "two frames later", s.next(), e, SAME_FACTS, STEADY);
    // ... and the other branch of the V pass's rule: a second pass within one frame
    expect("a second V pass within the frame", "the pass", "reflectionV", s.vPass(), true, "reflectionV: the previous reflection V pass was THIS FRAME'S or the frame before's"); }
  { Sim s; const uint32_t e = steady(s, "fused: steady state");      // a fused temporal pass
    s.fuse = true;
    static const Want FUSED = {true, SECOND.vWhy, false, "temporal: it keeps them on whole frames of the TWO-KERNEL path", false, NEW_EPOCH.skipWhy, false, "(the fused path has no tone map of its own)"};
    for (int k = 0; k < 3; ++k) check("a fused temporal pass", "fused frames", s.next(), e, SAME_FACTS, FUSED);
    s.fuse = false;
    static const Want AFTER = {true, SECOND.vWhy, true, SECOND.wordsWhy, false, SECOND.skipWhy,
                               false, "backBufferWrittenElsewhere: the back buffer has another writer than the tone map the record describes"};
    check("a fused temporal pass", "two kernels again", s.next(), e, SAME_FACTS, AFTER);
    check("a fused temporal pass", "one frame later", s.next(), e, SAME_FACTS, STEADY);
    // ... and the one sequence in which ONLY the invalidated record says no: within one frame a fused pass, an empty strip's denoise and a
    // two-kernel pass -- the tone map behind them has the parity, the frame and the write count the record of the frame before asks for
    ++s.frame; s.gen();
    s.fuse = true; s.denoise(); s.fuse = false;
    s.parity ^= 1u;
    expect("fused, then two kernels within one frame", "the second pass", "temporal keepsWords", s.denoise().words, true, SECOND.wordsWhy);
    expect("fused, then two kernels within one frame", "the tone map", "toneMap", s.tone(), false, AFTER.tmWhy); }
  { Sim s; const uint32_t e = steady(s, "other source: steady state");      // a tone map from another source (rtggx_present_accumulation)
    ++s.frame;
    expect("a tone map from another source", "that frame", "the epoch", s.gen(), e, SAME_FACTS);
    const Sim::Denoise d = s.denoise();
    expect("a tone map from another source", "that frame", "temporal maySkip", d.skip, true, STEADY.skipWhy);
    expect("a tone map from another source", "that frame", "toneMap", s.tone(false), false, "toneMap: for the image this tone map reads (TSS[parity], not another source: fromTss)");
    static const Want AFTER = {true, SECOND.vWhy, true, SECOND.wordsWhy, true, STEADY.skipWhy, false, "toneMap: the tone map before this one ... read the OTHER HISTORY IMAGE (it read another source)"};
    check("a tone map from another source", "one frame later", s.next(), e, SAME_FACTS, AFTER);
    check("a tone map from another source", "two frames later", s.next(), e, SAME_FACTS, STEADY); }
  { Sim s; const uint32_t e = steady(s, "empty strip: steady state");      // an empty strip's rtggx_denoise: the parity flips, no pass runs
    s.parity ^= 1u;
    static const Want AFTER = {true, SECOND.vWhy, true, SECOND.wordsWhy,
                               false, "temporal: ... and wrote the OTHER history image and word array (the caller's parity flips even for an empty strip's rtggx_denoise)",
                               false, "toneMap: the tone map before this one ... read the OTHER history image"};
    check("an empty strip's denoise", "the next frame", s.next(), e, SAME_FACTS, AFTER);
    check("an empty strip's denoise", "one frame later", s.next(), e, SAME_FACTS, STEADY); }
  { Sim s; const uint32_t e = steady(s, "fltRfl: steady state");      // FilteredOut written as well, then FilteredOut1 alone again
    static const Want OTHER_IMAGES = {false, "reflectionV: ... and wrote the same images (FilteredOut as well, or FilteredOut1 alone: fltRflIsFltDff)", true, SECOND.wordsWhy, true, STEADY.skipWhy, true, SECOND.tmWhy};
    s.diffuse = true; check("fltRfl non-null", "the event's frame", s.next(), e, SAME_FACTS, OTHER_IMAGES); check("fltRfl non-null", "one frame later", s.next(), e, SAME_FACTS, STEADY);
    s.diffuse = false; check("fltRfl null", "the event's frame", s.next(), e, SAME_FACTS, OTHER_IMAGES); check("fltRfl null", "one frame later", s.next(), e, SAME_FACTS, STEADY); }
}

static void scriptSwitches() {
  Sim s; uint32_t e = steady(s, "switches: steady state");
  static const Want NONE = {false, "the switches: with still sky off ... no pass may skip", false, "the switches: settled sky needs still sky", false, NEW_EPOCH.skipWhy, false, NEW_EPOCH.tmWhy};
  s.chain.enableStaticSky(false); ++e;
  expect("still sky off", "threshold", "prevRunThreshold", s.chain.prevRunThreshold(PREV_RUN, RUN_CAP), RUN_CAP + 1u, "with still sky off one more than a run can reach");
  for (int k = 0; k < 4; ++k) check("still sky off", "every frame", s.next(), e, "the switches: with still sky off the runs are still counted [under one epoch]", NONE);
  s.chain.enableStaticSky(true);
  expect("still sky on", "threshold", "prevRunThreshold", s.chain.prevRunThreshold(PREV_RUN, RUN_CAP), PREV_RUN, "RT_SKY_PREV_RUN");
  e = recover(s, "still sky on", e, "SkyBreak::FeatureSwitch");
  static const Want V_ONLY = {true, SECOND.vWhy, false, "the switches: with settled sky off no words are kept", false, NEW_EPOCH.skipWhy, false, "the switches: ... and neither the temporal pass nor the tone map leaves a block alone"};
  s.chain.enableSettledSky(false); ++e;
  check("settled sky off", "the event's frame", s.next(), e, "SkyBreak::FeatureSwitch", NEW_EPOCH);
  for (int k = 0; k < 3; ++k) check("settled sky off", "later frames", s.next(), e, SAME_FACTS, V_ONLY);
  s.chain.enableSettledSky(true);
  e = recover(s, "settled sky on", e, "SkyBreak::FeatureSwitch");
}

// The stale-history guard: the one sequence in which ONLY the count of writes says no.  After the tone map of frame f (it read TSS[p]) the
// denoiser runs twice more within frame f -- the passes write TSS[p ^ 1], then TSS[p] -- and frame f + 1 follows as usual.  Its tone map
// meets every other term: its own temporal pass kept words (and even left blocks alone), the tone map before it was frame f's, under the
// same epoch, over the same rows, of the other parity.  But TSS[p], the image the words compare with, is no longer what that tone map read.
// Second table: with the count undone (SkyChainProbe) the same step, "frame f + 1 / toneMap", answers yes -- that step alone is what
// deleting tssWrites would flip.
static void scriptStaleHistory() {
  Sim s; const uint32_t e = steady(s, "stale history: steady state");
  const uint32_t p = s.parity;
  for (int k = 0; k < 2; ++k) {
    const Sim::Denoise d = s.denoise();
    expect("stale history", "two more passes in frame f", "reflectionV", d.v, true, "reflectionV: the previous reflection V pass was THIS FRAME'S or the frame before's");
    expect("stale history", "two more passes in frame f", "temporal keepsWords", d.words, true, SECOND.wordsWhy);
    expect("stale history", "two more passes in frame f", "temporal maySkip", d.skip, false, "temporal: the temporal pass before this one was the PREVIOUS FRAME'S");
  }
  expect("stale history", "two more passes in frame f", "the parity", s.parity, p, "(two flips)");
  ++s.frame;
  expect("stale history", "frame f + 1", "the epoch", s.gen(), e, SAME_FACTS);
  const Sim::Denoise d = s.denoise();
  expect("stale history", "frame f + 1", "temporal keepsWords", d.words, true, SECOND.wordsWhy);
  expect("stale history", "frame f + 1", "temporal maySkip", d.skip, true, STEADY.skipWhy);
  Sim without = s;
  expect("stale history", "frame f + 1", "toneMap", s.tone(), false, "toneMap: read the OTHER history image AS IT STILL IS (no temporal pass has written it since: as many writes of TSS[parity ^ 1] now as when that tone map read it)");
  --rt::SkyChainProbe::tssWrites(without.chain, p);      // the one write of TSS[p] since frame f's tone map, uncounted
  expect("stale history, the count undone", "frame f + 1", "toneMap", without.tone(), true, "every other term of toneMap's rule holds: only the count says no");
  check("stale history", "frame f + 2", s.next(), e, SAME_FACTS, STEADY);
}

// The epoch's wrap: 2^24 - 1 bumps from the first epoch.
static void scriptWrap() {
  SkyChain c;
  expect("wrap", "a new chain", "the epoch", c.epoch(), 1, "the epoch starts at 1 (0 is what cleared words carry)");
  uint32_t most = 0; bool early = false;
  for (uint32_t k = 0; k + 1u < (1u << 24); ++k) {
    if (k + 2u == (1u << 24)) early = c.takeWrapped();      // (asked once before the last bump)
    c.breakRuns(SkyBreak::Upload);
    if (c.epoch() > most) most = c.epoch();
  }
  expect("wrap", "before the last bump", "takeWrapped", early, false, "takeWrapped: the epoch has wrapped since this was last asked: not yet");
  expect("wrap", "after 2^24 - 1 bumps", "the epoch", c.epoch(), 0, "the epoch: 24 bits ... once in 2^24 bumps it comes round to 0");
  expect("wrap", "after 2^24 - 1 bumps", "the largest epoch seen", most, 0xFFFFFF, "the epoch: 24 bits (a word is epoch << 8 | run or flags)");
  expect("wrap", "after 2^24 - 1 bumps", "takeWrapped", c.takeWrapped(), true, "takeWrapped: the epoch has wrapped since this was last asked");
  expect("wrap", "asked again", "takeWrapped", c.takeWrapped(), false, "takeWrapped: ... SINCE THIS WAS LAST ASKED");

  // A record made under the numerically equal epoch of the time round before.  2^24 bumps within one frame, between its ray generation and
  // its denoiser, bring the epoch back to the very value every record carries: the host's rules cannot tell, and license the skips.
  // FINDING, behaviour kept as it was before the chain was gathered here: the device words are cleared by the NEXT ray generation
  // (takeWrapped), not before.  Unreachable in practice -- sixteen million entry-point calls within one frame.
  Sim s; const uint32_t e = steady(s, "wrap: steady state");
  ++s.frame;
  expect("wrap within a frame", "ray generation", "the epoch", s.gen(), e, SAME_FACTS);
  for (uint32_t k = 0; k < (1u << 24); ++k) s.chain.breakRuns(SkyBreak::Upload);
  expect("wrap within a frame", "after 2^24 bumps", "the epoch", s.chain.epoch(), e, "24 bits: the same number again");
  const Sim::Denoise d = s.denoise();
  expect("wrap within a frame", "the frame's denoiser", "reflectionV", d.v, true, "FINDING (kept): genValidFor compares numbers, and the number is the same");
  expect("wrap within a frame", "the frame's denoiser", "temporal maySkip", d.skip, true, "FINDING (kept): as above");
  expect("wrap within a frame", "the frame's tone map", "toneMap", s.tone(), true, "FINDING (kept): as above");
  expect("wrap within a frame", "the next ray generation", "takeWrapped", (++s.frame, s.gen(), s.chain.takeWrapped()), true, "takeWrapped: launchRayTrace asks after rayGeneration and clears every word");
  // across a frame boundary nothing is licensed before the next ray generation: the record is another frame's
  Sim t; steady(t, "wrap: steady state");
  for (uint32_t k = 0; k < (1u << 24); ++k) t.chain.breakRuns(SkyBreak::Upload);
  ++t.frame;
  const Sim::Denoise d2 = t.denoise();
  expect("wrap between frames", "a denoiser before any ray generation", "reflectionV", d2.v, false, "genValidFor: THIS frame's ray generation has run");
  expect("wrap between frames", "a denoiser before any ray generation", "temporal maySkip", d2.skip, false, "genValidFor: THIS frame's ray generation has run");
  expect("wrap between frames", "its tone map", "toneMap", t.tone(), true, "FINDING (kept): the tone map's rule asks for this frame's temporal pass, not for its ray generation");
}

int main() {
  scriptEpochEvents();
  scriptRows();
  scriptBrokenChains();
  scriptSwitches();
  scriptStaleHistory();
  scriptWrap();
  if (g_failed) { std::printf("sky chain: %d of %d checks FAILED\n", g_failed, g_checked); return 1; }
  std::printf("sky chain: all %d checks passed\n", g_checked);
  return 0;
}
