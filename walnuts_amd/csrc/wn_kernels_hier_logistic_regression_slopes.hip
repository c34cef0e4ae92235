// the hier_logistic_regression_slopes device model (models/hier_slopes_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_slopes_glm.h"
#define WN_MODEL_ID 33
#define WN_MODEL_TAG hier_logistic_regression_slopes
#define WN_MODEL_TYPE wn::HierLogisticRegressionSlopesModel
#include "wn_kernels.inc"
