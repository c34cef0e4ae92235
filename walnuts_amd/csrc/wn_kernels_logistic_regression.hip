// the logistic_regression device model (models/glm.h): kernels for the one-wavefront geometries + registry entry
#include "models/glm.h"
#define WN_MODEL_ID 5
#define WN_MODEL_TAG logistic_regression
#define WN_MODEL_TYPE wn::LogisticRegressionModel
#include "wn_kernels.inc"
