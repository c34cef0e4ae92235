// wn_monitor.h -- the host side's share of the cross-chain monitors, common to the engine (wn_engine_elementwise.hip) and the
// sampling driver's controllers (wn_sample.hip).
#pragma once

#include <cmath>

namespace wn {

// R-hat of the log density over n chains (sampler.hpp:139-145) from the sum of the chains' sample variances and the
// sum of squared deviations of their means from the mean of means
inline double rhat_from_sums(double sum_of_variances, double sum_sq_dev, double n) {
  const double variance_of_means = sum_sq_dev / (n - 1);  // util.hpp:401-404
  const double mean_of_variances = sum_of_variances / n;
  return std::sqrt(1 + variance_of_means / mean_of_variances);  // sampler.hpp:145
}

}  // namespace wn
