// the hier_logistic_regression device model (models/hier_glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/hier_glm.h"
#define WN_MODEL_ID 16
#define WN_MODEL_TAG hier_logistic_regression
#define WN_MODEL_TYPE wn::HierLogisticRegressionModel
#include "wn_kernels.inc"
