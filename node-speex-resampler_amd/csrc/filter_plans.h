// filter_plans.h -- which kernel plans a filter gets and which of them a launch takes, each stated once (host only,
// product code).  build_tables (engine.cpp) uploads the rows of the plans plan_filter made, Batch::launch_chunk launches
// what choose_launch chose, and the speexhip_debug_plan / _plan64 / _launch_shape hooks (c_api.cpp) report from the same
// two functions: there is no second statement of either rule.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace speexhip {

// The plans of the period kernel a filter can have, in the order their tap rows are uploaded.
enum PeriodVariant : uint8_t {
  kBase,         // primary fast path (kernels_period.hip), R = 10 or 5
  kFine,         // the same filter with 5 phases per wave: launches of one generation take it beside an R = 10 kBase
  kW16,          // ... over an int16 LDS window (wide windows; int16 calls; .usable only where it pays)
  kPp,           // phase pairs (up to three channels, wide windows): chosen per launch (kernels_period_pp.hip)
  kPpW16,        // ... over an int16 LDS window
  kPeriod64,     // kBase with an fp64 accumulator (kernels_period64.hip): filters of the reference's double kinds
  kFine64,       // ... its R = 5 companion
  kPeriod64W16,  // ... over an int16 LDS window (kernels_period64_w16.hip)
  kPeriodVariants
};
inline bool is_double_kind(const FilterSpec &f) { return f.kind == kDirectDouble || f.kind == kInterpolateDouble; }

struct FilterPlans {
  PeriodPlan period[kPeriodVariants];  // a variant the filter does not have is !usable
  SlidePlan slide;                     // small-ratio fast path (kernels_slide.hip): usable only where kBase is not
  SlidePlan slide64;                   // ... with an fp64 accumulator: what FAST runs for the double kinds there
  ExactGeometry geo, geo_ch;           // exact kernel, all channels / one channel per launch
  // a variant whose tap rows go to the device (kBase without a float window only stands for its kW16 plan: no rows)
  bool has_rows(int v) const { return period[v].usable && (v != kBase || period[v].float_ok); }
};

// Every plan of the designed filter `f` for `channels` channels.  Returns the filter the period plans were made on, which
// is what their rows are built from (build_period_rows): `f` itself, or *folded -- the folded view of a ratio with
// den <= 6 outside the slide kernel's shapes (7:6 as 35:30, 11:1 as 110:10 ...: kernels.h, period_view), filled only then.
const FilterSpec &plan_filter(const FilterSpec &f, uint32_t channels, size_t lds_budget, FilterPlans *plans, FilterSpec *folded);

// What one launch of up to 32 stream descriptors runs.
enum class KernelFamily : uint8_t { Zero, Exact, Period, Slide, Slide64 };
struct LaunchChoice {
  KernelFamily family;
  PeriodVariant variant;  // Period: the plan of the launch
  bool with_fine;         // Period: the R = 5 companion `fine` goes along (launch_period takes it for a single generation)
  PeriodVariant fine;
  bool float_io;          // the sample type the launcher is given (an int16-window launch is always an int16 one)
};
// mode = SPEEXHIP_MODE_*; zero_mode = resampler_basic_zero is installed; float_seen = the histories may hold samples an
// int16 window cannot; w16_override: -1 none, 0 never, 1 always the int16-window plan where one exists (diagnostics).
// Allocates nothing: this is on the path of every launch.
LaunchChoice choose_launch(const FilterPlans &p, const FilterSpec &f, int mode, bool zero_mode, bool float_io, bool float_seen,
                           int w16_override, const StreamDesc *descs, uint32_t n);

}  // namespace speexhip
