// the hier_linear_regression_sigma_centered device model (models/hier_scale_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_scale_glm.h"
#define WN_MODEL_ID 36
#define WN_MODEL_TAG hier_linear_regression_sigma_centered
#define WN_MODEL_TYPE wn::HierLinearRegressionSigmaCenteredModel
#include "wn_kernels.inc"
