// fast_atan2.hip.h -- OpenCV's fastAtan2: the degree-7 odd polynomial on [0, 1] unfolded over the octants, in float; degrees in
// [0, 360).  Shared by the ORB orientation (orb_cv.hip) and the SIFT orientation / descriptor histograms (sift.hip).
#pragma once

__device__ __forceinline__ float fast_atan2_deg(float y, float x)
{
    const float k = (float)(180 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k, p5 = 0.1555786518463281f * k,
                p7 = -0.04432655554792128f * k;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)2.2204460492503131e-16);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)2.2204460492503131e-16);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0)
        a = 180.f - a;
    if (y < 0)
        a = 360.f - a;
    return a;
}
