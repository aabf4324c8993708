// filter_plans.cpp -- see filter_plans.h.
#include "filter_plans.h"

#include "diag.h"

namespace speexhip {

const FilterSpec &plan_filter(const FilterSpec &f, uint32_t channels, size_t lds_budget, FilterPlans *plans, FilterSpec *folded) {
  FilterPlans &t = *plans;
  t = FilterPlans();
  PeriodPlan *p = t.period;
  static const bool no_fine = SPEEXHIP_DIAG_ENV("SPEEXHIP_NO_FINE") != nullptr;  // diagnostics: A/B
  t.geo = exact_geometry(f, channels, lds_budget);
  t.geo_ch = exact_geometry(f, 1, lds_budget);
  // (ratios with den <= 6 outside the slide kernel's shapes -- 7:6, 11:1, 16:3 ... -- plan the period kernel on a folded
  //  view of the filter, 35:30, 110:10, 80:15: kernels.h, period_view; `pf` is what every period plan below is made on)
  const FilterSpec &pf = period_view(f, channels, folded) ? *folded : f;
  p[kBase] = plan_period(pf, channels, lds_budget);
  if (p[kBase].usable && p[kBase].float_ok && p[kBase].r == 10) {
    p[kFine] = plan_period_r(pf, channels, lds_budget, 5);
    // (... and a float window of its own: an R = 5 plan that only stands for its int16 plan -- 100 channels of 320:147, one
    //  period per tile either way -- has nothing to launch; found by the fuzzer the day the layouts without an ISA loop
    //  got int16 plans, seed 611002591)
    if (no_fine || !p[kFine].float_ok || p[kFine].lane_periods != p[kBase].lane_periods) p[kFine].usable = false;
  }
  p[kW16] = plan_period_w16(pf, channels, lds_budget, p[kBase]);
  if (p[kBase].usable && period_wants_pp_plans(pf, channels)) {
    p[kPp] = plan_period(pf, channels, lds_budget, false, false, true);
    if (p[kPp].usable) p[kPpW16] = plan_period_w16(pf, channels, lds_budget, p[kPp]);
  }
  t.slide = plan_slide(f, channels);
  if (p[kBase].usable) t.slide.usable = false;  // (the period kernel serves: no rows, nothing to launch)
  // the reference's double kinds (quality 9, 10): fp64-accumulate twins of the fast kernels
  if (is_double_kind(f)) {
    if (p[kBase].usable) {
      p[kPeriod64] = plan_period(pf, channels, lds_budget, false, true);
      if (p[kPeriod64].usable && p[kPeriod64].r == 10) {
        p[kFine64] = plan_period_r(pf, channels, lds_budget, 5, false, true);
        if (no_fine || p[kFine64].lane_periods != p[kPeriod64].lane_periods) p[kFine64].usable = false;
      }
    }
    if (p[kPeriod64].usable) p[kPeriod64W16] = plan_period_w16(pf, channels, lds_budget, p[kPeriod64]);
    if (t.slide.usable) t.slide64 = plan_slide64(f, channels);
  }
  return pf;
}

// The kernel for one launch: what the mode, the filter's plans and the launch's size select.
LaunchChoice choose_launch(const FilterPlans &t, const FilterSpec &f, int mode, bool zero_mode, bool float_io, bool float_seen,
                           int w16_override, const StreamDesc *descs, uint32_t n) {
  const PeriodPlan *p = t.period;
  const bool fast = mode != SPEEXHIP_MODE_EXACT;
  // the fast path sums in fp64 (mode FAST or FAST_FIXED on a filter the reference sums in fp64)
  const bool acc64 = (mode == SPEEXHIP_MODE_FAST || mode == SPEEXHIP_MODE_FAST_FIXED) && is_double_kind(f);
  const bool i16_window = !float_io && !float_seen;  // the histories hold PCM values and so does this call's input
  const bool w16_always = w16_override == 1, w16_never = w16_override == 0;
  LaunchChoice c = {KernelFamily::Exact, kBase, false, kFine, float_io};
  auto period = [&c](PeriodVariant v) {
    c.family = KernelFamily::Period;
    c.variant = v;
  };
  if (zero_mode) {
    c.family = KernelFamily::Zero;
  } else if (fast && acc64 && p[kPeriod64].usable && i16_window && p[kPeriod64W16].usable && !w16_never &&
             (w16_always || period_launch_prefers_w16(f, p[kPeriod64], p[kFine64].usable, descs, n))) {
    // ... over an int16 LDS window where the float window holds a fraction of a tile (wide windows; round 5)
    period(kPeriod64W16);
    c.float_io = false;
  } else if (fast && acc64 && p[kPeriod64].usable) {
    // the reference sums these filters in fp64 (resample.c:389-435, :501-558): v_fma_f64 kernels
    period(kPeriod64);
    c.with_fine = p[kFine64].usable;
    c.fine = kFine64;
  } else if (fast && acc64 && !p[kBase].usable && t.slide64.usable) {
    c.family = KernelFamily::Slide64;
  } else if (fast && p[kPp].usable &&
             period_launch_prefers_pp(f, (i16_window && p[kW16].usable) ? p[kW16] : p[kBase],
                                      (i16_window && p[kPpW16].usable) ? p[kPpW16] : p[kPp], descs, n)) {
    // up to three channels, wide windows: phase pairs (lane = (period, channel), half the window per tile) where this
    // launch gains
    period((i16_window && p[kPpW16].usable) ? kPpW16 : kPp);
  } else if (fast && p[kBase].usable && i16_window && p[kW16].usable &&
             (w16_always || period_launch_prefers_w16(f, p[kBase], p[kFine].usable, descs, n))) {
    // wide windows: twice the periods per tile over an int16 LDS image (the histories hold PCM values) -- unless
    // the launch is too small for that to pay (period_launch_prefers_w16)
    period(kW16);
    c.float_io = false;
  } else if (fast && p[kBase].usable && p[kBase].float_ok) {
    period(kBase);
    c.with_fine = p[kFine].usable;
  } else if (fast && t.slide.usable) {
    c.family = KernelFamily::Slide;
  }
  return c;
}

}  // namespace speexhip
