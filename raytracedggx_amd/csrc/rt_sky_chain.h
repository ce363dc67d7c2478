// Still sky and settled sky: the host's whole argument for letting a kernel leave pixels alone, in one place and without HIP (plain
// C++17; a stream is a const void*), so that tests/sky_chain_main.cpp can drive it on a CPU.  DESIGN.md section 5.
//
// Four passes may leave work undone over sky that has stopped changing: ray generation and the reflection V pass ("still sky", by the
// tiles' run words, InputSet::skyRun), the temporal pass and the tone map ("settled sky", by the blocks' settled words,
// rtggx_context::settled).  All four rest on one argument: a pass may leave a block alone only if the PREVIOUS pass of its kind stored the
// same bits there, into the same image, under the same epoch.  Where the argument has a hole the result is a silently stale image, not a
// crash.  SkyChain keeps the facts of the most recent pass of each kind and the epoch; every pass asks it through the one method named
// after it, handing over the facts of THIS pass, and gets the decision back.  The method records "now" as "was" itself, after it has
// decided: no caller can get that order wrong.  The decisions only select kernel arguments and template variants (the launchers say
// which); the constants the kernels share with the host (RT_SKY_PREV_RUN, RT_SKY_V_RUN, RT_SETTLED_*) stay in rtggx_context.h.
#pragma once
#include <cstdint>
#include <cstring>

namespace rt {

// What ends every run, and why: the single list.  A run says "the tile had no surface in so many consecutive ray generations, and
// nothing its outputs depend on changed meanwhile"; the epoch is bumped -- every run starts again from 0, every tile is written in full
// for RT_SKY_PREV_RUN frames, every settled word reads as unsettled -- by SkyChain::rayGeneration from what it can compare frame to
// frame (Generation), and by breakRuns(reason) from the entry points that change the rest.  The reason changes nothing at run time; the
// most recent one is kept for a debugger.  Tile words that fall back to "all ones" (a foreign or uploaded visibility buffer, a
// traversal-bound frame) need no entry here: every tile reads as drawn, which ends its run.
enum class SkyBreak : uint8_t {
  None,                // nothing has ended the runs yet
  Generation,          // rayGeneration: this ray generation differs from the one before it (the list is above that method)
  Environment,         // rtggx_set_env, rtggx_set_env_image, rtggx_generate_env_mips, rtggx_prefilter_env: the sky behind every pixel is another
                       //   one (of the last two: every level below the first); a failed build has left the old one and ends nothing
  Upload,              // rtggx_upload: what a still-sky tile relies on being in place may just have been replaced (TSS, FilteredOut1 and
                       //   the back buffer included: whatever is written behind the kernels' back)
  Strip,               // rtggx_set_strip: other rows, and tiles count from the pass's first row
  TraceRays,           // rtggx_trace_rays: it refills a set's bins, and a still-sky tile relies on its bins' counts being 0
  SetBuffers,          // allocSet, at creation and when growBins has released the bins: a set with new buffers, nothing is in place in it
  TileWordsSwitch,     // rtggx_debug_tile_words: which tiles read as drawn changes
  FeatureSwitch,       // rtggx_debug_static_sky, rtggx_debug_settled_sky: no run or word from before the switch is relied on after it
};

class SkyChain {
 public:
  // ---- the switches (rtggx_debug_static_sky, rtggx_debug_settled_sky).  With still sky off the runs are still counted, but no run is
  // ever long enough (prevRunThreshold) and no pass may skip; with settled sky off no words are kept and neither the temporal pass nor
  // the tone map leaves a block alone.  Settled sky needs still sky: its kernels read the run words.
  void enableStaticSky(bool on) { staticSky_ = on; breakRuns(SkyBreak::FeatureSwitch); }
  void enableSettledSky(bool on) { settledSky_ = on; breakRuns(SkyBreak::FeatureSwitch); }

  // ---- the epoch: 24 bits (a word is epoch << 8 | run or flags), bumped whenever something a sky tile's outputs depend on changes or
  // the chain of consecutive ray generations breaks (SkyBreak).  Once in 2^24 bumps it comes round to 0: no word of an earlier time
  // round may meet its epoch again, so the next ray generation clears every word on the device (takeWrapped).
  void breakRuns(SkyBreak why) { epoch_ = (epoch_ + 1u) & 0xFFFFFFu; if (epoch_ == 0u) wrapped_ = true; lastBreak_ = why; }
  // "the epoch has wrapped since this was last asked": launchRayTrace asks after rayGeneration and keeps the device-side consequences
  bool takeWrapped() { const bool w = wrapped_; wrapped_ = false; return w; }

  // ---- read-only, for the launchers' kernel arguments and for debug.hip (rtggx_debug_sky_runs, rtggx_debug_settled_words)
  uint32_t epoch() const { return epoch_; }
  uint32_t genTilesX() const { return gen_.tilesX; }      // the tile grid of the most recent ray generation
  uint32_t genTilesY() const { return gen_.tilesY; }
  SkyBreak lastBreak() const { return lastBreak_; }
  // the run from which ray generation leaves a tile alone: RT_SKY_PREV_RUN, or with still sky off one more than a run can reach
  uint32_t prevRunThreshold(uint32_t prevRun, uint32_t runCap) const { return staticSky_ ? prevRun : runCap + 1u; }

  // ---- ray generation (rayGenKernel): the epoch this frame's ray generation counts its tiles' runs under (rtggx_context.h
  // InputSet::skyRun, RT_SKY_PREV_RUN).  The epoch is bumped when this ray generation differs from the one before it in anything that
  // enters a sky pixel's outputs or the bookkeeping the skipped epilogue keeps:
  //     the camera        rg.ProjToWorld, rg.EyePt, compared bit for bit (the sample rebuilds them from the same matrices every frame and
  //                       changes them when the user drags the mouse; the jitter, the frame index and the model's turn do not enter)
  //     the frame before  was not a ray generation's: a set in the ring went by without one (rtggx_render_visibility alone), so "the
  //                       previous set" is not the previous ray generation's (a second ray generation within one frame is fine)
  //     the rows          another strip: tiles count from the pass's first row
  //     the bins          ray rate, adaptive split on / off, slice shift: which bins a tile has, and whether the cost records are kept
  //     the stream        the previous set's words are ordered before this kernel by stream order only
  // and the very first one has none before it.  -DRT_SKY_NO_CAMERA_CHECK leaves the camera out: tests/test_gpu_static_sky.py must fail
  // with it (and does).
  struct GenFacts {
    uint32_t frame = 0, rows[2] = {0, 0}, rate = 0, sliceShift = 0, tilesX = 0, tilesY = 0;
    bool adaptive = false;
    const void* stream = nullptr;
    float camera[20] = {};      // ProjToWorld, EyePt
  };
  uint32_t rayGeneration(const GenFacts& now) {
    const GenFacts& was = gen_;
    bool same = genAny_ && (was.frame == now.frame || was.frame + 1u == now.frame) && was.rows[0] == now.rows[0] && was.rows[1] == now.rows[1]
                && was.rate == now.rate && was.adaptive == now.adaptive && was.sliceShift == now.sliceShift && was.stream == now.stream;
#ifndef RT_SKY_NO_CAMERA_CHECK
    same = same && std::memcmp(was.camera, now.camera, sizeof now.camera) == 0;
#endif
    if (!same) breakRuns(SkyBreak::Generation);
    gen_ = now; genAny_ = true; genEpoch_ = epoch_;
    return epoch_;
  }

  // ---- the reflection V pass (spatialTiledKernel<1>): may this frame's pass leave blocks over still sky alone?  It may when what it
  // would store there is what the PREVIOUS reflection V pass stored, into the same image:
  //     this frame's ray generation has run (genValidFor);
  //     the previous reflection V pass was this frame's or the frame before's (a frame without rtggx_denoise leaves FilteredOut1 a frame
  //       old), had ray generation's results of its own frame under the same epoch, covered the same rows and wrote the same images
  //       (FilteredOut as well, or FilteredOut1 alone: fltRflIsFltDff).
  // The direct-access variant of the kernel converts every sky texel whatever the answer; it counts as the previous pass all the same.
  struct VFacts { uint32_t frame = 0, gbufferRow0 = 0, rows[2] = {0, 0}; bool fltRflNull = false; };
  bool reflectionV(const VFacts& now) {
    const bool genValid = genValidFor(now.frame, now.gbufferRow0);
    const uint32_t genEpoch = genValid ? genEpoch_ : 0xFFFFFFFFu;
    const bool may = staticSky_ && genValid && vAny_ && (v_.frame == now.frame || v_.frame + 1u == now.frame) && vGenEpoch_ == genEpoch
                     && v_.rows[0] == now.rows[0] && v_.rows[1] == now.rows[1] && v_.fltRflNull == now.fltRflNull;
    v_ = now; vAny_ = true; vGenEpoch_ = genEpoch;
    return may;
  }

  // ---- the temporal pass (temporalKernel): does this frame's pass keep settled words, and may it leave blocks alone for the words of
  // the pass before it?  It keeps them on whole frames (no strip: no histReach, no peers, no apron rows) of the two-kernel path, at
  // least six tiles across (temporalKernel's loads), when the pass before it ran under the same epoch.  Under a NEW epoch it stores none
  // and needs none: every word in either array carries an older epoch and reads as unsettled (a camera that moves every frame pays
  // nothing).  The first pass after anything else that breaks the chain -- a fused pass, a frame without the denoiser -- stores
  // `epoch | 0` everywhere, over words that may describe images written since.
  // It may leave blocks alone when, besides,
  //     this frame's ray generation has run (genValidFor, as the reflection V pass requires it);
  //     the temporal pass before this one was the previous frame's, kept words, over the same rows, and wrote the other history image
  //       and word array (the caller's parity flips even for an empty strip's rtggx_denoise, which runs no pass).
  // Whatever it does, it is recorded as the previous pass of the next, and counted as a write of TSS[parity] (toneMap).
  struct TemporalFacts { uint32_t frame = 0, gbufferRow0 = 0, rows[2] = {0, 0}, parity = 0, width = 0; bool fused = false, whole = false; };
  struct TemporalDecision { bool keepsWords, maySkip; };
  TemporalDecision temporal(const TemporalFacts& now) {
    const bool words = staticSky_ && settledSky_ && !now.fused && now.whole && now.width >= 96u && tAny_ && tEpoch_ == epoch_;
    const bool may = words && genValidFor(now.frame, now.gbufferRow0) && tWords_ && t_.frame + 1u == now.frame && t_.parity == (now.parity ^ 1u)
                     && t_.rows[0] == now.rows[0] && t_.rows[1] == now.rows[1];
    t_ = now; tAny_ = true; tWords_ = words; tEpoch_ = epoch_;
    ++tssWrites_[now.parity & 1u];
    return {words, may};
  }

  // ---- the fused path (temporalToneKernel): the back buffer has another writer than the tone map the record describes
  void backBufferWrittenElsewhere() { tmAny_ = false; }

  // ---- the tone map (toneMapKernel): it may leave blocks alone for this frame's words when
  //     this frame's temporal pass kept words, for the image this tone map reads (TSS[parity], not another source: fromTss), under the
  //       epoch that is still current;
  //     the tone map before this one was the previous frame's, under the same epoch, over the same rows, and read the OTHER history image
  //       as it still is (no temporal pass has written it since: as many writes of TSS[parity ^ 1] now as when that tone map read it):
  //       the image this frame's words compare with.
  struct ToneMapFacts { uint32_t frame = 0, rows[2] = {0, 0}, parity = 0; bool fromTss = false, whole = false; };
  bool toneMap(const ToneMapFacts& now) {
    const bool may = staticSky_ && settledSky_ && now.whole && now.fromTss && tAny_ && tWords_ && t_.frame == now.frame && t_.parity == now.parity && tEpoch_ == epoch_
                     && tmAny_ && tm_.fromTss && tm_.frame + 1u == now.frame && tmEpoch_ == epoch_ && tm_.rows[0] == now.rows[0] && tm_.rows[1] == now.rows[1]
                     && tm_.parity == (now.parity ^ 1u) && tmWrites_ == tssWrites_[(now.parity ^ 1u) & 1u];
    tm_ = now; tmAny_ = true; tmEpoch_ = epoch_; tmWrites_ = tssWrites_[now.parity & 1u];
    return may;
  }

 private:
  friend struct SkyChainProbe;      // tests/sky_chain_main.cpp: shows which term of a rule says no by undoing that term alone
  // This frame's ray generation has run under the epoch that is still current (nothing has broken the runs since: an upload, another
  // environment, ...), over the rows the run words are indexed by -- the words in this set are this frame's.
  bool genValidFor(uint32_t frame, uint32_t row0) const { return genAny_ && gen_.frame == frame && genEpoch_ == epoch_ && gen_.rows[0] == row0; }

  bool staticSky_ = true, settledSky_ = true;
  uint32_t epoch_ = 1u; bool wrapped_ = false; SkyBreak lastBreak_ = SkyBreak::None;
  // the facts of the most recent pass of each kind (xAny_: there has been one), and what the chain itself knew when it ran
  GenFacts gen_; bool genAny_ = false; uint32_t genEpoch_ = 0;
  VFacts v_; bool vAny_ = false; uint32_t vGenEpoch_ = 0;                              // (vGenEpoch_: all ones where its frame's ray generation was not valid)
  TemporalFacts t_; bool tAny_ = false, tWords_ = false; uint32_t tEpoch_ = 0;
  ToneMapFacts tm_; bool tmAny_ = false; uint32_t tmEpoch_ = 0, tmWrites_ = 0;          // (tmWrites_: tssWrites_[its parity] when it read that image)
  uint32_t tssWrites_[2] = {0, 0};      // temporal passes that have written TSS[p]
};

}  // namespace rt
