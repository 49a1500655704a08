/*
 * mfm_ais.h - the message half of the reference's AIS decoder, fed by the GPU AIS stage.
 *
 * ais/ais_decode.h gives a front end three calls: ais_decode_new(&d, freq, on_position_report,
 * on_base_station_report, on_static_voyage_data), ais_decode_on_pcm(d, pcm, n), ais_decode_delete(&d).  Here the
 * sample-rate work of on_pcm (slicer, preamble detector, NRZI / HDLC bit recovery, FCS) runs on the GPU for all
 * channels at once (mfm_ais_*, include/multifm_hip.h) and hands back one event per candidate packet; what is left
 * is _ais_decode_demod_on_msg and the three report decoders (ais/ais_decode.c:74-289).  Same object name, report
 * structs, callback and constructor signatures; ais_decode_on_events() takes the place of ais_decode_on_pcm().
 *
 * Two deliberate deviations from the reference:
 *   - Short packets.  A packet whose FCS holds but which is too short for the fields of its type makes the
 *     reference abort (TSL_BUG_ON in _ais_decode_get_bitfield, ais_decode.c:34).  Here it is dropped and counted
 *     (ais_decode_short_packets).
 *   - rawAscii length.  The reference armours the packet into a 199-byte buffer four characters at a time, so from
 *     148-byte packets on it writes past the buffer and hands it on unterminated.  Here rawAscii stops at the 196
 *     characters (49 groups, 147 bytes) the reference forms within bounds.
 */
#pragma once

#include <multifm_hip.h>

#include "mfm_tsl.h"

struct ais_decode;

/* ais/ais_decode.h:7-53 */
struct ais_position_report {
    uint32_t mmsi;
    uint32_t nav_stat;
    uint32_t position_acc;
    uint32_t course;
    uint32_t heading;
    uint32_t timestamp;

    float longitude;
    float latitude;

    int32_t rate_of_turn;
    float speed_over_ground;
};

struct ais_base_station_report {
    uint32_t mmsi;
    uint32_t year;
    uint32_t month;
    uint32_t day;
    uint32_t hour;
    uint32_t minute;
    uint32_t second;

    float longitude;
    float latitude;

    uint32_t epfd_type;
    const char *epfd_name;
};

struct ais_static_voyage_data {
    uint32_t mmsi;
    uint32_t version;
    uint32_t imo_number;
    uint32_t ship_type;
    uint32_t dim_to_bow;
    uint32_t dim_to_stern;
    uint32_t dim_to_port;
    uint32_t dim_to_starboard;
    uint32_t fix_type;
    const char *epfd_name;
    uint32_t eta_month;
    uint32_t eta_day;
    uint32_t eta_hour;
    uint32_t eta_minute;
    float draught;
    char callsign[8];
    char ship_name[21];
    char destination[21];
};

/* ais/ais_decode.h:55-57 */
typedef aresult_t (*ais_decode_on_position_report_func_t)(struct ais_decode *decode, void *state,
                                                          struct ais_position_report *rpt, const char *raw_msg);
typedef aresult_t (*ais_decode_on_base_station_report_func_t)(struct ais_decode *decode, void *state,
                                                              struct ais_base_station_report *bsr, const char *raw_msg);
typedef aresult_t (*ais_decode_on_static_voyage_data_func_t)(struct ais_decode *decode, void *state,
                                                             struct ais_static_voyage_data *svd, const char *raw_msg);

/* ais/ais_decode.h:59-60; freq is stored and, as in the reference, not used */
aresult_t ais_decode_new(struct ais_decode **pdecode, uint32_t freq, ais_decode_on_position_report_func_t on_position_report,
                         ais_decode_on_base_station_report_func_t on_base_station_report,
                         ais_decode_on_static_voyage_data_func_t on_static_voyage_data);
aresult_t ais_decode_delete(struct ais_decode **pdecode);

/* the events of ONE channel, in stream order (mfm_ais_fetch_events returns them grouped by channel).  Events with
 * fcs_valid = 0 are counted as CRC rejects (ais_demod.c:201) and produce nothing. */
aresult_t ais_decode_on_events(struct ais_decode *decode, const struct mfm_ais_event *events, size_t nr_events);

/* packets rejected by the FCS check so far (struct ais_demod::crc_rejects) */
size_t ais_decode_crc_rejects(const struct ais_decode *decode);
/* CRC-valid packets dropped because they were too short for their message type (see above) */
size_t ais_decode_short_packets(const struct ais_decode *decode);

/* opaque user pointer for the callbacks (the reference's callbacks reach their state through globals; they get
 * NULL as `state`, as in ais_decode.c:107,176,249) */
void ais_decode_set_user(struct ais_decode *decode, void *user);
void *ais_decode_get_user(struct ais_decode *decode);
