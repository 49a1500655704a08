/*
 * ais_restatement.c - a sequential restatement of the AIS receive chain, for the tests only:
 *
 *   demod    one 48 kHz sample at a time, as ais/ais_demod.c:114-258 does it (five preamble registers, NRZI,
 *            unstuffing, end flag / 1280-bit cut, CRC-16) - one event per packet end with >= 4 bytes
 *   decode   message types 1-5 as ais/ais_decode.c:21-289 decodes them
 *   json     the three JSON lines of decoder/decoder.c:320-394, with the time fixed at the epoch
 *
 * Written from the behaviour of those functions, with the two deviations the host layer documents: a packet
 * whose CRC holds but which is too short for its type is dropped and counted (the reference aborts), and
 * rawAscii stops at 196 characters (the reference writes past its buffer from 148-byte packets on).
 *
 * Built by tests/ais_ref.py with gcc into a temporary directory; used through ctypes.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct ais_r_event { /* struct mfm_ais_event */
    uint32_t channel;
    uint32_t fcs_valid;
    uint32_t nr_bytes;
    uint32_t reserved;
    uint64_t sample;
    uint64_t start_sample;
    uint8_t bytes[160];
};

/* ---- demod ------------------------------------------------------------------------------------------------ */

/* CRC-16 bit by bit: reflected 0x8408, register starts at all ones, result inverted (ais_demod.c:19-36) */
uint16_t ais_r_crc16(const uint8_t *p, size_t n)
{
    uint16_t r = 0xffff;
    for (size_t k = 0; k < n; k++) {
        r ^= p[k];
        for (int b = 0; b < 8; b++) {
            r = (r & 1) ? (uint16_t)((r >> 1) ^ 0x8408) : (uint16_t)(r >> 1);
        }
    }
    return (uint16_t)~r;
}

struct ais_r {
    uint32_t reg[5];   /* detector shift registers, one per sample phase (ais_demod_priv.h:25) */
    uint8_t prev[5];   /* last slice seen by each phase */
    unsigned phase;    /* the register the next sample updates */
    int receiving;
    unsigned skip;     /* sample counter while receiving; a bit is read when skip % 5 == 0 (:227) */
    uint8_t pkt[800];  /* ais_demod_priv.h:80 */
    uint8_t shr;       /* last eight raw bits, newest in bit 0 */
    uint8_t last;      /* slice of the previous read sample */
    unsigned nbits;    /* bits written */
    unsigned ones;     /* consecutive ones read, since the rx reset */
    uint64_t n;        /* samples consumed */
    uint64_t start;
    uint64_t crc_rejects;
};

static void detector_clear(struct ais_r *d)
{
    memset(d->reg, 0, sizeof(d->reg));
    memset(d->prev, 0, sizeof(d->prev));
    d->phase = 0;
}

static void rx_clear(struct ais_r *d)
{
    memset(d->pkt, 0, sizeof(d->pkt));
    d->shr = 0;
    d->nbits = 0;
    d->ones = 0;
}

struct ais_r *ais_r_new(void)
{
    struct ais_r *d = calloc(1, sizeof(*d));
    if (d) {
        detector_clear(d);
        rx_clear(d);
    }
    return d;
}

void ais_r_free(struct ais_r *d)
{
    free(d);
}

uint64_t ais_r_crc_rejects(const struct ais_r *d)
{
    return d->crc_rejects;
}

static int popcount32(uint32_t v)
{
    int c = 0;
    while (v) {
        v &= v - 1;
        c++;
    }
    return c;
}

/* returns 1 when a preamble is found on this sample (:114-158) */
static int detect(struct ais_r *d, int16_t s)
{
    const uint8_t now = s > 0;
    const uint8_t before = d->prev[d->phase];
    d->prev[d->phase] = now;
    d->reg[d->phase] = (d->reg[d->phase] << 1) | (uint32_t)(before == now);
    int hits = 0;
    for (int k = 0; k < 5; k++) {
        hits += popcount32(d->reg[k] ^ 0x5555557eu) <= 2;
    }
    const int found = hits >= 3;
    if (found) {
        d->receiving = 1;
        d->skip = 2;
        rx_clear(d);
        d->last = now;
    }
    d->phase = (d->phase + 1) % 5;
    return found;
}

/* one read bit (:160-213); returns 1 when the packet ended, *ev filled when it was a candidate */
static int rx_bit(struct ais_r *d, int16_t s, struct ais_r_event *ev, int *emitted)
{
    const uint8_t now = s > 0;
    const uint8_t bit = d->last == now;
    d->shr = (uint8_t)((d->shr << 1) | bit);
    d->last = now;
    if (d->ones < 5) {
        d->pkt[d->nbits / 8] |= (uint8_t)(bit << (d->nbits % 8));
        d->nbits++;
    }
    d->ones = bit ? d->ones + 1 : 0;
    *emitted = 0;
    if (d->shr != 0x7e && d->nbits != 1280) {
        return 0;
    }
    const unsigned nb = d->nbits / 8;
    if (nb >= 4) {
        const uint16_t want = ais_r_crc16(d->pkt, nb - 2);
        const uint16_t got = (uint16_t)(d->pkt[nb - 2] | (d->pkt[nb - 1] << 8));
        memset(ev, 0, sizeof(*ev));
        ev->fcs_valid = want == got;
        ev->nr_bytes = nb;
        ev->sample = d->n;
        ev->start_sample = d->start;
        memcpy(ev->bytes, d->pkt, 160);
        if (!ev->fcs_valid) {
            d->crc_rejects++;
        }
        *emitted = 1;
    }
    d->receiving = 0;
    detector_clear(d);
    return 1;
}

/* consume n samples; writes up to max events, returns how many there were */
size_t ais_r_feed(struct ais_r *d, const int16_t *pcm, size_t n, uint32_t channel, struct ais_r_event *out, size_t max)
{
    size_t ne = 0;
    for (size_t i = 0; i < n; i++, d->n++) {
        if (!d->receiving) {
            if (detect(d, pcm[i])) {
                d->start = d->n;
            }
        } else if ((d->skip++ % 5) == 0) {
            struct ais_r_event ev;
            int emitted = 0;
            rx_bit(d, pcm[i], &ev, &emitted);
            if (emitted) {
                ev.channel = channel;
                if (ne < max) {
                    out[ne] = ev;
                }
                ne++;
            }
        }
    }
    return ne;
}

/* ---- decode + JSON ---------------------------------------------------------------------------------------- */

/* big-endian bit field of a packet of len bytes; -1 when it does not fit (ais_decode.c:21-46 aborts there) */
static int64_t field(const uint8_t *p, size_t len, size_t off, size_t bits)
{
    const size_t first = off / 8, last = (off + bits + 7) / 8;
    if (last > len) {
        return -1;
    }
    uint64_t a = 0;
    for (size_t k = first; k < last; k++) {
        a = (a << 8) | p[k];
    }
    a >>= last * 8 - (off + bits);
    return (int64_t)(a & ((1ull << bits) - 1));
}

static int32_t sfield(int64_t v, size_t bits)
{
    const uint32_t u = (uint32_t)v << (32 - bits);
    return (int32_t)u >> (32 - bits);
}

static const char *const EPFD[16] = { "Undefined", "GPS", "GLONASS", "Combined GPS/GLONASS", "Loran-C", "Chayka",
    "Integrated Navigation System", "Surveyed", "Galileo", "Unknown 9", "Unknown 10", "Unknown 11", "Unknown 12",
    "Unknown 13", "Unknown 14", "Unknown 15" };

struct sink {
    char *buf;
    size_t cap, len;
};

static void put(struct sink *s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#include <stdarg.h>
static void put(struct sink *s, const char *fmt, ...)
{
    char tmp[2048];
    va_list ap;
    va_start(ap, fmt);
    const int k = vsnprintf(tmp, sizeof(tmp), fmt, ap);
    va_end(ap);
    for (int i = 0; i < k; i++) {
        if (s->len + 1 < s->cap) {
            s->buf[s->len] = tmp[i];
        }
        s->len++;
    }
    if (s->cap) {
        s->buf[s->len < s->cap ? s->len : s->cap - 1] = '\0';
    }
}

/* decoder.c:121-166 */
static void put_escaped(struct sink *s, const char *t)
{
    for (; *t; t++) {
        const char ch = *t;
        switch (ch) {
        case '\n':
        case '\r': put(s, "\\n"); break;
        case '"': put(s, "\\\""); break;
        case '\\': put(s, "\\\\"); break;
        case '/': put(s, "\\/"); break;
        case '\b': put(s, "<BKSP>"); break;
        case '\f': put(s, "<FF>"); break;
        case '\t': put(s, "\\t"); break;
        case 0x03:
        case 0x04:
        case 0x17: put(s, " "); break;
        default:
            if (ch >= 0x20 && ch < 0x7f) {
                put(s, "%c", ch);
            } else {
                put(s, "\\u%04x", (unsigned)ch);
            }
        }
    }
}

static void text6(const uint8_t *p, size_t len, size_t off, size_t nch, char *dst)
{
    for (size_t i = 0; i < nch; i++) {
        const int v = (int)field(p, len, off + 6 * i, 6);
        dst[i] = (char)(v > 0x1f ? v : v + 0x40);
    }
    dst[nch] = '\0';
}

#define TS "\"timestamp\":\"1970-01-01 00:00:00 UTC\","

/*
 * Decode the events of one channel into JSON lines.  stats[0] += CRC rejects, stats[1] += CRC-valid packets too
 * short for their type, stats[2] += lines written.  Returns the length the whole text needs.
 */
size_t ais_r_json(const struct ais_r_event *ev, size_t n, char *out, size_t cap, uint64_t *stats)
{
    struct sink s = { out, cap, 0 };
    if (cap) {
        out[0] = '\0';
    }
    for (size_t e = 0; e < n; e++) {
        if (!ev[e].fcs_valid) {
            stats[0]++;
            continue;
        }
        const uint8_t *p = ev[e].bytes;
        const size_t len = ev[e].nr_bytes - 2;
        /* ASCII armour, three bytes -> four characters (ais_decode.c:218-268), at most 49 groups */
        char armour[197];
        size_t na = 0;
        for (size_t off = 0; off < len && na + 4 <= 196; off += 3) {
            uint32_t acc = 0;
            for (size_t j = off; j < off + 3 && j < len; j++) {
                acc = (acc << 8) | p[j];
            }
            for (int j = 0; j < 4; j++) {
                const unsigned v = (acc >> (18 - 6 * j)) & 0x3f;
                armour[na++] = (char)(v <= 39 ? v + 48 : v - 40 + 96);
            }
        }
        armour[na] = '\0';
        const unsigned type = (p[0] >> 2) & 0x3f;
        const uint32_t mmsi = ((uint32_t)p[1] << 22) | ((uint32_t)p[2] << 14) | ((uint32_t)p[3] << 6) | ((uint32_t)p[4] >> 2);
        size_t need;
        switch (type) {
        case 1: case 2: case 3: need = 18; break;
        case 4: need = 18; break;
        case 5: need = 53; break;
        default: continue; /* nothing for other types */
        }
        if (len < need) {
            stats[1]++;
            continue;
        }
        if (type <= 3) {
            const unsigned nav = (unsigned)field(p, len, 38, 4);
            const int32_t rot = sfield(field(p, len, 42, 8), 8);
            const float sog = (float)(uint32_t)field(p, len, 50, 10) / 10.0;
            const unsigned acc = (unsigned)field(p, len, 60, 1);
            const float lon = (float)sfield(field(p, len, 61, 28), 28) / 600000.0;
            const float lat = (float)sfield(field(p, len, 89, 27), 27) / 600000.0;
            const unsigned course = (unsigned)field(p, len, 116, 12);
            const unsigned heading = (unsigned)field(p, len, 128, 9);
            const unsigned secs = (unsigned)field(p, len, 137, 6);
            put(&s, "{\"proto\":\"ais\",\"type\":\"positionReport\"," TS
                    "\"mmsi\":%u,\"navStat\":%u,\"rateOfTurn\":%d,\"speedOverGround\":%f,\"positionAcc\":%u,"
                    "\"geoPosition\":{\"lon\":%f,\"lat\":%f},\"course\":%u,\"heading\":%u,\"seconds\":%u,\"rawAscii\":\"",
                mmsi, nav, rot, (double)sog, acc, (double)lon, (double)lat, course, heading, secs);
        } else if (type == 4) {
            const unsigned y = (unsigned)field(p, len, 38, 14), mo = (unsigned)field(p, len, 52, 4),
                           d = (unsigned)field(p, len, 56, 5), h = (unsigned)field(p, len, 61, 5),
                           mi = (unsigned)field(p, len, 66, 6), se = (unsigned)field(p, len, 72, 6);
            const float lon = (float)sfield(field(p, len, 79, 28), 28) / 600000.0;
            const float lat = (float)sfield(field(p, len, 107, 27), 27) / 600000.0;
            const unsigned epfd = (unsigned)field(p, len, 134, 4);
            put(&s, "{\"proto\":\"ais\",\"type\":\"baseStationReport\"," TS
                    "\"mmsi\":%u,\"baseStationDate\":\"%04u-%02u-%02u %02u:%02u:%02u UTC\","
                    "\"geoPosition\":{\"lon\":%f,\"lat\":%f},\"fixType\":\"%s\",\"rawAscii\":\"",
                mmsi, y, mo, d, h, mi, se, (double)lon, (double)lat, EPFD[epfd & 15]);
        } else {
            char call[8], name[21], dest[21];
            const unsigned ver = (unsigned)field(p, len, 38, 2), imo = (unsigned)field(p, len, 40, 30);
            text6(p, len, 70, 7, call);
            text6(p, len, 112, 20, name);
            const unsigned st = (unsigned)field(p, len, 232, 8), bow = (unsigned)field(p, len, 240, 9),
                           stern = (unsigned)field(p, len, 249, 9), port = (unsigned)field(p, len, 258, 6),
                           stb = (unsigned)field(p, len, 264, 6), fix = (unsigned)field(p, len, 270, 4),
                           em = (unsigned)field(p, len, 274, 4), ed = (unsigned)field(p, len, 278, 5),
                           eh = (unsigned)field(p, len, 283, 5), emi = (unsigned)field(p, len, 288, 6);
            const float draught = (float)(uint32_t)field(p, len, 294, 8) / 10.0;
            text6(p, len, 302, 20, dest);
            put(&s, "{\"proto\":\"ais\",\"type\":\"staticAndVoyageData\"," TS
                    "\"mmsi\":%u,\"version\":%u,\"imoNumber\":%u,\"callsign\":\"%s\",\"shipName\":\"%s\","
                    "\"shipType\":%u,\"dimensions\":{\"toBow\":%u,\"toStern\":%u,\"toPort\":%u,\"toStarboard\":%u},"
                    "\"fixType\":\"%s\",\"eta\":\"%02u-%02u %02u:%02u\",\"draught\":%f,\"destination\":\"%s\","
                    "\"rawAscii\":\"",
                mmsi, ver, imo, call, name, st, bow, stern, port, stb, EPFD[fix & 15], em, ed, eh, emi, (double)draught,
                dest);
        }
        put_escaped(&s, armour);
        put(&s, "\"}\n");
        stats[2]++;
    }
    return s.len;
}
