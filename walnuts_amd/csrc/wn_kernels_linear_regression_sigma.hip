// the linear_regression_sigma device model (models/glm_scale.h): kernels for the one-wavefront geometries + registry entry
#include "models/glm_scale.h"
#define WN_MODEL_ID 26
#define WN_MODEL_TAG linear_regression_sigma
#define WN_MODEL_TYPE wn::LinearRegressionSigmaModel
#include "wn_kernels.inc"
