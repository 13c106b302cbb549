// The sun's elevation and azimuth for a date, time and place: computeSunEA
// (skysun/SunLocation.cpp:17-104; Blanco-Muriel et al., "Computing the Solar
// Vector", Solar Energy 70(5), 2001) in double precision as the reference
// runs it, with its float constants (Pi, Deg2Rad) and its (float) cast of the
// sidereal angle.  Angles in radians, Y up (ElevationAzimuth.h).
#pragma once

#include <cmath>

namespace igx {

struct SunTime { // TimePoint (SunLocation.h:8-15): 2020-05-06 12:00:00
    int year = 2020, month = 5, day = 6, hour = 12, minute = 0;
    float seconds = 0.0f;
};
struct SunPlace { // MapLocation (SunLocation.h:32-35): Saarbruecken
    float longitude = -6.9965744f; // degrees west
    float latitude = 49.235422f;   // degrees north
    float timezone = -2;           // offset to UTC
};
struct ElevationAzimuth {
    float elevation; // above the horizon
    float azimuth;   // west of south
};

inline ElevationAzimuth compute_sun_ea(const SunTime& t, const SunPlace& p) {
    constexpr float Pi = 3.14159265358979323846f, Pi2 = 1.57079632679489661923f, Deg2Rad = Pi / 180.0f;
    constexpr double EARTH_MEAN_RADIUS = 6371.01, ASTRONOMICAL_UNIT = 149597890;
    const double dec_hours = t.hour + p.timezone + (t.minute + t.seconds / 60.0) / 60.0;
    const int aux1 = (t.month - 14) / 12;
    const int aux2 = (1461 * (t.year + 4800 + aux1)) / 4 + (367 * (t.month - 2 - 12 * aux1)) / 12 -
                     (3 * ((t.year + 4900 + aux1) / 100)) / 4 + t.day - 32075;
    const double julian_date = (double)aux2 - 0.5 + dec_hours / 24.0;
    const double days = julian_date - 2451545.0;

    const double omega = 2.1429 - 0.0010394594 * days;
    const double mean_longitude = 4.8950630 + 0.017202791698 * days;
    const double anomaly = 6.2400600 + 0.0172019699 * days;
    const double ecl_longitude = mean_longitude + 0.03341607 * std::sin(anomaly) + 0.00034894 * std::sin(2 * anomaly) - 0.0001134 -
                                 0.0000203 * std::sin(omega);
    const double ecl_obliquity = 0.4090928 - 6.2140e-9 * days + 0.0000396 * std::cos(omega);

    const double sin_ecl = std::sin(ecl_longitude);
    double right_ascension = std::atan2(std::cos(ecl_obliquity) * sin_ecl, std::cos(ecl_longitude));
    if (right_ascension < 0) right_ascension += 2 * Pi;
    const double declination = std::asin(std::sin(ecl_obliquity) * sin_ecl);

    const double gmst = 6.6974243242 + 0.0657098283 * days + dec_hours;
    const double lmst = Deg2Rad * ((float)((gmst * 15 - p.longitude)));
    const double lat = Deg2Rad * p.latitude;
    const double cos_lat = std::cos(lat), sin_lat = std::sin(lat);
    const double hour_angle = lmst - right_ascension;
    const double cos_hour = std::cos(hour_angle);
    double zenith = std::acos(cos_lat * cos_hour * std::cos(declination) + std::sin(declination) * sin_lat);
    double azimuth = std::atan2(-std::sin(hour_angle), std::tan(declination) * cos_lat - sin_lat * cos_hour);
    if (azimuth < 0) azimuth += 2 * Pi;
    zenith += (EARTH_MEAN_RADIUS / ASTRONOMICAL_UNIT) * std::sin(zenith); // parallax
    // east of north -> west of south
    return ElevationAzimuth{Pi2 - (float)zenith, std::fmod((float)azimuth + Pi, 2 * Pi)};
}

} // namespace igx
