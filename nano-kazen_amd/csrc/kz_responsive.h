// kz_responsive.h - what kz_denoise.hip (the host path of every denoise call) and kz_responsive.hip (the two kernels of include/kazen_mi355x_responsive.h, which
// holds the definition) share on the host. Nothing here is an argument of a kernel: what kz_dn_prepare_responsive takes by value (KzDnTemporal, KzDnMotion, KzDnFast)
// is kz_denoise.h's and kz_history.h's, beside the one body of the stage that the three history kernels instantiate.
#pragma once
#include "../../include/kazen_mi355x_responsive.h"
#include "kz_denoise.h"

// What kz_denoise_responsive adds to a call, beside KzDnMotion in KzDnVar (a host struct): the checked options with the defaults in, and the fast plane's two
// copies - inF the one the taps read (null: ABSENT, the taps read the history's (e, v) in its place), outF the one the pixel's (f, vf) goes to.
struct KzDnResponsive { float fastHistory, clampSigma; int radius; bool clampOff; const float4 *inF; float4 *outF; };

// The launches of the stage on `stream` (kz_responsive.hip): kz_dn_prepare_responsive in kz_dn_prepare_motion's place (M.ids null: every pixel static), and behind
// it kz_dn_clamp_history over colour, T.outE and T.outN - pass B, launched only where it can change a pixel: with a history to read and without CLAMP_OFF.
int kzDnResponsiveRun(int width, int height, int border, const float4 *film, const float4 *moment, const float4 *albedo, const float4 *normal, const float4 *depth,
                      int demodulate, float samples, const KzDnTemporal &T, const KzDnMotion &M, const KzDnResponsive &R, float4 *colour, float4 *normalZ,
                      float4 *albedoP, hipStream_t stream);
