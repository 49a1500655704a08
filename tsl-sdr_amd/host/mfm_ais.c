/*
 * mfm_ais.c - see mfm_ais.h.  Packets arrive FCS-checked from the GPU stage (one mfm_ais_event per packet end with
 * at least four bytes); what is done here is ais_decode.c:21-289 on the ones whose FCS holds.
 */
#include "mfm_ais.h"

#include <string.h>

#define AIS_ARMOUR_CHARS 196 /* 49 groups of four: what fits in the reference's char[(168 + 4 * 256 + 5) / 6] */

struct ais_decode {
    uint32_t freq;
    ais_decode_on_position_report_func_t on_position_report;
    ais_decode_on_base_station_report_func_t on_base_station_report;
    ais_decode_on_static_voyage_data_func_t on_static_voyage_data;
    void *user;
    size_t crc_rejects;
    size_t short_packets;
};

/* ais_decode.c:21-46: len bits at bit offset `offset`, MSB first across bytes.  The callers check the length first. */
static uint32_t get_bitfield(const uint8_t *packet, size_t offset, size_t len)
{
    const size_t start_byte = offset / 8, end_byte = (offset + len + 7) / 8;
    uint64_t acc = 0;
    for (size_t i = start_byte; i < end_byte; i++) {
        acc <<= 8;
        acc |= packet[i];
    }
    acc >>= end_byte * 8 - (offset + len);
    acc &= (1ull << len) - 1;
    return (uint32_t)acc;
}

/* ais_decode.c:48-54 */
static int32_t get_bitfield_signed(const uint8_t *packet, size_t offset, size_t len)
{
    const uint32_t t = get_bitfield(packet, offset, len);
    const int32_t v = (int32_t)(t << (32 - len));
    return v >> (32 - len);
}

/* ais_decode.c:56-69: 6-bit text, v > 0x1f ? v : v + 0x40 */
static void get_string(const uint8_t *packet, size_t offset, size_t nr_chars, char *dest)
{
    for (size_t i = 0; i < nr_chars; i++) {
        const char v = (char)get_bitfield(packet, offset + 6 * i, 6);
        dest[i] = v > 0x1f ? v : v + 0x40;
    }
}

/* ais_decode.c:107-126 */
static const char *const epfd_type[16] = {
    "Undefined", "GPS", "GLONASS", "Combined GPS/GLONASS", "Loran-C", "Chayka", "Integrated Navigation System",
    "Surveyed", "Galileo", "Unknown 9", "Unknown 10", "Unknown 11", "Unknown 12", "Unknown 13", "Unknown 14", "Unknown 15",
};

/* ais_decode.c:71-105 (types 1-3) */
static void position_report(struct ais_decode *d, const uint8_t *p, uint32_t mmsi, const char *raw)
{
    struct ais_position_report rpt;
    memset(&rpt, 0, sizeof(rpt));
    rpt.mmsi = mmsi;
    rpt.nav_stat = get_bitfield(p, 38, 4);
    rpt.rate_of_turn = get_bitfield_signed(p, 42, 8);
    rpt.speed_over_ground = (float)get_bitfield(p, 50, 10) / 10.0;
    rpt.position_acc = get_bitfield(p, 60, 1);
    rpt.longitude = (float)get_bitfield_signed(p, 61, 28) / 600000.0;
    rpt.latitude = (float)get_bitfield_signed(p, 89, 27) / 600000.0;
    rpt.course = get_bitfield(p, 116, 12);
    rpt.heading = get_bitfield(p, 128, 9);
    rpt.timestamp = get_bitfield(p, 137, 6);
    if (NULL != d->on_position_report) {
        d->on_position_report(d, NULL, &rpt, raw);
    }
}

/* ais_decode.c:128-163 (type 4) */
static void base_station_report(struct ais_decode *d, const uint8_t *p, uint32_t mmsi, const char *raw)
{
    struct ais_base_station_report bsr;
    memset(&bsr, 0, sizeof(bsr));
    bsr.mmsi = mmsi;
    bsr.year = get_bitfield(p, 38, 14);
    bsr.month = get_bitfield(p, 52, 4);
    bsr.day = get_bitfield(p, 56, 5);
    bsr.hour = get_bitfield(p, 61, 5);
    bsr.minute = get_bitfield(p, 66, 6);
    bsr.second = get_bitfield(p, 72, 6);
    bsr.longitude = (float)get_bitfield_signed(p, 79, 28) / 600000.0;
    bsr.latitude = (float)get_bitfield_signed(p, 107, 27) / 600000.0;
    bsr.epfd_type = get_bitfield(p, 134, 4);
    bsr.epfd_name = epfd_type[bsr.epfd_type & 0xf];
    if (NULL != d->on_base_station_report) {
        d->on_base_station_report(d, NULL, &bsr, raw);
    }
}

/* ais_decode.c:165-216 (type 5) */
static void static_voyage_data(struct ais_decode *d, const uint8_t *p, uint32_t mmsi, const char *raw)
{
    struct ais_static_voyage_data asd;
    memset(&asd, 0, sizeof(asd));
    asd.mmsi = mmsi;
    asd.version = get_bitfield(p, 38, 2);
    asd.imo_number = get_bitfield(p, 40, 30);
    get_string(p, 70, 7, asd.callsign);
    asd.callsign[7] = '\0';
    get_string(p, 112, 20, asd.ship_name);
    asd.ship_name[20] = '\0';
    asd.ship_type = get_bitfield(p, 232, 8);
    asd.dim_to_bow = get_bitfield(p, 240, 9);
    asd.dim_to_stern = get_bitfield(p, 249, 9);
    asd.dim_to_port = get_bitfield(p, 258, 6);
    asd.dim_to_starboard = get_bitfield(p, 264, 6);
    asd.fix_type = get_bitfield(p, 270, 4);
    asd.epfd_name = epfd_type[asd.fix_type & 0xf];
    asd.eta_month = get_bitfield(p, 274, 4);
    asd.eta_day = get_bitfield(p, 278, 5);
    asd.eta_hour = get_bitfield(p, 283, 5);
    asd.eta_minute = get_bitfield(p, 288, 6);
    asd.draught = (float)get_bitfield(p, 294, 8) / 10.0;
    get_string(p, 302, 20, asd.destination);
    asd.destination[20] = '\0';
    if (NULL != d->on_static_voyage_data) {
        d->on_static_voyage_data(d, NULL, &asd, raw);
    }
}

/* ais_decode.c:218-226 */
static char to_ascii_armor(uint8_t in)
{
    return in <= 39 ? (char)(in + 48) : (char)(in - 40 + 96);
}

/* ais_decode.c:229-289, for a packet of packet_len bytes whose FCS holds */
static void on_msg(struct ais_decode *d, const uint8_t *packet, size_t packet_len)
{
    char msg_ascii_6[AIS_ARMOUR_CHARS + 1];
    memset(msg_ascii_6, 0, sizeof(msg_ascii_6));
    /* three bytes -> four characters; a last group of one or two bytes is not padded, its value sits in the low
     * bits of the accumulator (ais_decode.c:247-258) */
    size_t offs = 0;
    for (size_t i = 0; i < AIS_ARMOUR_CHARS && offs < packet_len; i += 4) {
        uint32_t accum = 0;
        for (size_t j = offs; j < offs + 3 && j < packet_len; j++) {
            accum <<= 8;
            accum |= packet[j];
        }
        offs += 3;
        for (size_t j = 0; j < 4; j++) {
            msg_ascii_6[i + j] = to_ascii_armor((accum >> ((3 - j) * 6)) & 0x3f);
        }
    }
    const unsigned msg_id = (packet[0] >> 2) & 0x3f;
    /* bytes needed by the last field each report reads: 143 bits (types 1-3), 138 (type 4), 422 (type 5) */
    size_t need = 0;
    switch (msg_id) {
    case 1:
    case 2:
    case 3:
    case 4:
        need = 18;
        break;
    case 5:
        need = 53;
        break;
    default:
        return; /* the reference decodes nothing else */
    }
    if (packet_len < need) {
        d->short_packets++; /* the reference aborts here (ais_decode.c:34) */
        return;
    }
    uint32_t mmsi = (uint32_t)packet[1] << 22;
    mmsi |= (uint32_t)packet[2] << 14;
    mmsi |= (uint32_t)packet[3] << 6;
    mmsi |= ((uint32_t)packet[4] >> 2) & 0x3f;
    if (msg_id <= 3) {
        position_report(d, packet, mmsi, msg_ascii_6);
    } else if (4 == msg_id) {
        base_station_report(d, packet, mmsi, msg_ascii_6);
    } else {
        static_voyage_data(d, packet, mmsi, msg_ascii_6);
    }
}

aresult_t ais_decode_new(struct ais_decode **pdecode, uint32_t freq, ais_decode_on_position_report_func_t on_position_report,
                         ais_decode_on_base_station_report_func_t on_base_station_report,
                         ais_decode_on_static_voyage_data_func_t on_static_voyage_data)
{
    TSL_ASSERT_ARG(NULL != pdecode);
    struct ais_decode *d = calloc(1, sizeof(*d));
    if (NULL == d) {
        return A_E_NOMEM;
    }
    d->freq = freq;
    d->on_position_report = on_position_report;
    d->on_base_station_report = on_base_station_report;
    d->on_static_voyage_data = on_static_voyage_data;
    *pdecode = d;
    return A_OK;
}

aresult_t ais_decode_delete(struct ais_decode **pdecode)
{
    TSL_ASSERT_ARG(NULL != pdecode);
    TSL_ASSERT_ARG(NULL != *pdecode);
    free(*pdecode);
    *pdecode = NULL;
    return A_OK;
}

aresult_t ais_decode_on_events(struct ais_decode *decode, const struct mfm_ais_event *events, size_t nr_events)
{
    TSL_ASSERT_ARG(NULL != decode);
    TSL_ASSERT_ARG(NULL != events || 0 == nr_events);
    for (size_t i = 0; i < nr_events; i++) {
        const struct mfm_ais_event *ev = &events[i];
        if (ev->nr_bytes < 4 || ev->nr_bytes > sizeof(ev->bytes)) {
            return A_E_INVAL; /* the GPU stage never emits these */
        }
        if (!ev->fcs_valid) {
            decode->crc_rejects++; /* ais_demod.c:201 */
            continue;
        }
        on_msg(decode, ev->bytes, ev->nr_bytes - 2);
    }
    return A_OK;
}

size_t ais_decode_crc_rejects(const struct ais_decode *decode)
{
    return decode->crc_rejects;
}

size_t ais_decode_short_packets(const struct ais_decode *decode)
{
    return decode->short_packets;
}

void ais_decode_set_user(struct ais_decode *decode, void *user)
{
    decode->user = user;
}

void *ais_decode_get_user(struct ais_decode *decode)
{
    return decode->user;
}
