#include "myslam/types.h"
#include "myslam_shim/keyframe_db_hip.inl"
