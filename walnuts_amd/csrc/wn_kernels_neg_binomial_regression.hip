// the neg_binomial_regression device model (models/glm_scale.h): kernels for the one-wavefront geometries + registry entry
#include "models/glm_scale.h"
#define WN_MODEL_ID 25
#define WN_MODEL_TAG neg_binomial_regression
#define WN_MODEL_TYPE wn::NegBinomialRegressionModel
#include "wn_kernels.inc"
