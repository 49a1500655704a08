/*
 * aisdecoder_main.c - `aisdecoder_amd`: the reference's `decoder -m AIS` (decoder/decoder.c), batched.
 *
 * The reference runs one decoder process per channel FIFO: read int16 samples, optional inversion, polyphase
 * resampler, optional DC blocker, ais_decode_on_pcm, JSON lines (decoder.c:320-394, 580-673).  Here every input named
 * on the command line is one channel of a single GPU pipeline
 *
 *     PCM block (host) -> mfm_resampler (I/D, -b, -i) -> mfm_ais (slicer / preamble / bits / FCS)     on the MI355X
 *     events (host)    -> ais_decode_on_events -> position / base station / static and voyage -> JSON   per channel
 *
 * Same options and loop as decoder_amd (decoder_main.c): -I -D -S -F -f -o -c -b -p -i, plus -B block size, -g
 * device and -s (sign bits instead of PCM between resampler and AIS stage, not with -b; same JSON lines); several inputs are allowed (with more than one, -o NAME writes NAME.0, NAME.1, ...), read in lock step,
 * processing stops at the shortest.  The JSON lines are the reference's byte for byte, rawAscii through the same
 * escaper, callsign / ship name / destination unescaped (decoder.c:372).  MFM_DECODER_FIXED_TIME=1 prints the epoch
 * instead of the wall clock, so two runs can be diffed.  There is no CPU path: without a device it refuses.
 */
#include <errno.h>
#include <ctype.h>
#include <fcntl.h>
#include <inttypes.h>
#include <time.h>
#include <unistd.h>

#include "mfm_ais.h"
#include "mfm_config.h"

#define DEC_MSG(sev, sys, msg, ...) MESSAGE("DECODER", sev, sys, msg, ##__VA_ARGS__)
#define Q_15_SHIFT 14 /* filter/filter.h:16 */

struct chan {
    int fd;
    FILE *out;
    struct ais_decode *ais;
};

static bool g_fixed_time = false;

/* decoder.c:121-166 */
static void put_alnum_char(FILE *fp, char ch)
{
    switch (ch) {
    case '\n':
    case '\r':
        fprintf(fp, "\\n");
        break;
    case '\"':
        fprintf(fp, "\\\"");
        break;
    case '\\':
        fprintf(fp, "\\\\");
        break;
    case '/':
        fprintf(fp, "\\/");
        break;
    case '\b':
        fprintf(fp, "<BKSP>");
        break;
    case '\f':
        fprintf(fp, "<FF>");
        break;
    case '\t':
        fprintf(fp, "\\t");
        break;
    case 0x03:
    case 0x04:
    case 0x17:
        fprintf(fp, " ");
        break;
    default:
        if (isprint((unsigned char)ch)) {
            fprintf(fp, "%c", ch);
        } else {
            fprintf(fp, "\\u%04x", (unsigned)ch);
        }
    }
}

static struct tm *now_utc(void)
{
    static time_t now;
    now = g_fixed_time ? 0 : time(NULL);
    return gmtime(&now);
}

static void put_raw(FILE *fp, const char *raw_msg)
{
    for (size_t i = 0; i < strlen(raw_msg); i++) {
        put_alnum_char(fp, raw_msg[i]);
    }
    fprintf(fp, "\"}\n");
}

/* decoder.c:320-342 */
static aresult_t on_position_report(struct ais_decode *decode, void *state, struct ais_position_report *pr, const char *raw_msg)
{
    FILE *out = ((struct chan *)ais_decode_get_user(decode))->out;
    const struct tm *gmt = now_utc();
    fprintf(out,
            "{\"proto\":\"ais\",\"type\":\"positionReport\",\"timestamp\":\"%04i-%02i-%02i %02i:%02i:%02i UTC\","
            "\"mmsi\":%u,\"navStat\":%u,\"rateOfTurn\":%d,\"speedOverGround\":%f,\"positionAcc\":%u,"
            "\"geoPosition\":{\"lon\":%f,\"lat\":%f},\"course\":%u,\"heading\":%u,\"seconds\":%u,\"rawAscii\":\"",
            gmt->tm_year + 1900, gmt->tm_mon + 1, gmt->tm_mday, gmt->tm_hour, gmt->tm_min, gmt->tm_sec, pr->mmsi,
            pr->nav_stat, pr->rate_of_turn, (double)pr->speed_over_ground, pr->position_acc, (double)pr->longitude,
            (double)pr->latitude, pr->course, pr->heading, pr->timestamp);
    put_raw(out, raw_msg);
    return A_OK;
}

/* decoder.c:344-365 */
static aresult_t on_base_station_report(struct ais_decode *decode, void *state, struct ais_base_station_report *br,
                                        const char *raw_msg)
{
    FILE *out = ((struct chan *)ais_decode_get_user(decode))->out;
    const struct tm *gmt = now_utc();
    fprintf(out,
            "{\"proto\":\"ais\",\"type\":\"baseStationReport\",\"timestamp\":\"%04i-%02i-%02i %02i:%02i:%02i UTC\","
            "\"mmsi\":%u,\"baseStationDate\":\"%04u-%02u-%02u %02u:%02u:%02u UTC\","
            "\"geoPosition\":{\"lon\":%f,\"lat\":%f},\"fixType\":\"%s\",\"rawAscii\":\"",
            gmt->tm_year + 1900, gmt->tm_mon + 1, gmt->tm_mday, gmt->tm_hour, gmt->tm_min, gmt->tm_sec, br->mmsi, br->year,
            br->month, br->day, br->hour, br->minute, br->second, (double)br->longitude, (double)br->latitude, br->epfd_name);
    put_raw(out, raw_msg);
    return A_OK;
}

/* decoder.c:367-394; callsign, ship name and destination go out unescaped (the reference's TODO at :372) */
static aresult_t on_static_voyage_data(struct ais_decode *decode, void *state, struct ais_static_voyage_data *svd,
                                       const char *raw_msg)
{
    FILE *out = ((struct chan *)ais_decode_get_user(decode))->out;
    const struct tm *gmt = now_utc();
    fprintf(out,
            "{\"proto\":\"ais\",\"type\":\"staticAndVoyageData\",\"timestamp\":\"%04i-%02i-%02i %02i:%02i:%02i UTC\","
            "\"mmsi\":%u,\"version\":%u,\"imoNumber\":%u,\"callsign\":\"%s\",\"shipName\":\"%s\","
            "\"shipType\":%u,\"dimensions\":{\"toBow\":%u,\"toStern\":%u,\"toPort\":%u,\"toStarboard\":%u},"
            "\"fixType\":\"%s\",\"eta\":\"%02u-%02u %02u:%02u\",\"draught\":%f,\"destination\":\"%s\","
            "\"rawAscii\":\"",
            gmt->tm_year + 1900, gmt->tm_mon + 1, gmt->tm_mday, gmt->tm_hour, gmt->tm_min, gmt->tm_sec, svd->mmsi,
            svd->version, svd->imo_number, svd->callsign, svd->ship_name, svd->ship_type, svd->dim_to_bow,
            svd->dim_to_stern, svd->dim_to_port, svd->dim_to_starboard, svd->epfd_name, svd->eta_month, svd->eta_day,
            svd->eta_hour, svd->eta_minute, (double)svd->draught, svd->destination);
    put_raw(out, raw_msg);
    return A_OK;
}

static void usage(const char *app)
{
    DEC_MSG(SEV_INFO, "USAGE",
            "%s -I [interpolate] -D [decimate] -F [filter file] -S [input sample rate] -f [center freq] [-c] "
            "[-o output JSON file] [-b] [-p pole] [-i] [-s] [-B block samples] [-g gpu] in_fifo [in_fifo ...]",
            app);
    exit(EXIT_SUCCESS);
}

/* a whole block unless the input ends (FIFOs return short reads) */
static ssize_t read_full(int fd, void *buf, size_t bytes)
{
    size_t got = 0;
    while (got < bytes) {
        ssize_t r = read(fd, (char *)buf + got, bytes - got);
        if (r < 0) {
            if (EINTR == errno) {
                continue;
            }
            return -1;
        }
        if (0 == r) {
            break;
        }
        got += (size_t)r;
    }
    return (ssize_t)got;
}

int main(int argc, char *const argv[])
{
    unsigned interpolate = 1, decimate = 1, input_sample_rate = 0, center_freq = 0, block = 1u << 18;
    int device = 0, arg;
    bool dc_blocker = false, invert = false, create_out = false, sign_bits = false;
    double dc_block_pole = 0.9999;
    const char *filter_file = NULL, *out_file_name = NULL;

    while ((arg = getopt(argc, argv, "co:I:D:S:F:f:p:B:g:bish")) != -1) {
        switch (arg) {
        case 'o':
            out_file_name = optarg;
            break;
        case 'c':
            create_out = true;
            break;
        case 'f':
            center_freq = (unsigned)strtoll(optarg, NULL, 0);
            break;
        case 'I':
            interpolate = (unsigned)strtoll(optarg, NULL, 0);
            break;
        case 'D':
            decimate = (unsigned)strtoll(optarg, NULL, 0);
            break;
        case 'S':
            input_sample_rate = (unsigned)strtoll(optarg, NULL, 0);
            break;
        case 'F':
            filter_file = optarg;
            break;
        case 'b':
            dc_blocker = true;
            break;
        case 'p':
            dc_block_pole = strtod(optarg, NULL);
            break;
        case 'i':
            invert = true;
            break;
        case 's': /* resampler -> AIS stage as one sign bit per sample, no resampled PCM in device memory */
            sign_bits = true;
            break;
        case 'B':
            block = (unsigned)strtoll(optarg, NULL, 0);
            break;
        case 'g':
            device = (int)strtol(optarg, NULL, 0);
            break;
        case 'h':
        default:
            usage(argv[0]);
        }
    }
    g_fixed_time = NULL != getenv("MFM_DECODER_FIXED_TIME");
    if (optind >= argc) {
        DEC_MSG(SEV_FATAL, "MISSING-SRC-DEST", "Missing source file / FIFO");
        exit(EXIT_FAILURE);
    }
    if (0 == decimate || 0 == interpolate || 0 == block) {
        DEC_MSG(SEV_FATAL, "BAD-DECIMATION", "Interpolation, decimation and block size must be non-zero integers.");
        exit(EXIT_FAILURE);
    }
    if (0 == center_freq) {
        DEC_MSG(SEV_FATAL, "BAD-PAGER-FREQ", "Pager frequency must be non-zero");
        exit(EXIT_FAILURE);
    }
    if (sign_bits && dc_blocker) {
        DEC_MSG(SEV_FATAL, "BAD-SIGN-BIT-PATH", "The sign-bit path (-s) cannot be used with the DC blocker (-b): it filters the resampled PCM.");
        exit(EXIT_FAILURE);
    }
    if (NULL == filter_file) {
        DEC_MSG(SEV_FATAL, "BAD-FILTER-FILE", "Need to specify a filter JSON file.");
        exit(EXIT_FAILURE);
    }
    DEC_MSG(SEV_INFO, "CONFIG", "Resampling: %u/%u from %u to %f", interpolate, decimate, input_sample_rate,
            ((double)interpolate / (double)decimate) * (double)input_sample_rate);

    /* decoder.c:520-533: lpfCoeffs -> Q14 by truncation */
    struct config *cfg = NULL;
    double *coeffs_f = NULL;
    size_t nr_coeffs = 0;
    TSL_BUG_IF_FAILED(config_new(&cfg));
    if (FAILED(config_add(cfg, filter_file))) {
        DEC_MSG(SEV_INFO, "BAD-CONFIG", "Configuration file '%s' cannot be processed, aborting.", filter_file);
        exit(EXIT_FAILURE);
    }
    TSL_BUG_IF_FAILED(config_get_float_array(cfg, &coeffs_f, &nr_coeffs, "lpfCoeffs"));
    int16_t *coeffs = calloc(nr_coeffs, sizeof(int16_t));
    TSL_BUG_ON(NULL == coeffs);
    for (size_t i = 0; i < nr_coeffs; i++) {
        coeffs[i] = (int16_t)(coeffs_f[i] * (double)(1 << Q_15_SHIFT));
    }

    const unsigned nr_chan = (unsigned)(argc - optind);
    struct chan *ch = calloc(nr_chan, sizeof(*ch));
    TSL_BUG_ON(NULL == ch);
    for (unsigned c = 0; c < nr_chan; c++) {
        if (0 > (ch[c].fd = open(argv[optind + c], O_RDONLY))) {
            DEC_MSG(SEV_INFO, "BAD-INPUT", "Bad input - cannot open %s", argv[optind + c]);
            exit(EXIT_FAILURE);
        }
        if (NULL == out_file_name) {
            ch[c].out = stdout;
        } else {
            char name[4096];
            if (1 == nr_chan) {
                snprintf(name, sizeof(name), "%s", out_file_name);
            } else {
                snprintf(name, sizeof(name), "%s.%u", out_file_name, c);
            }
            if (NULL == (ch[c].out = fopen(name, create_out ? "w+" : "a"))) {
                DEC_MSG(SEV_INFO, "BAD-OUTPUT-FILE", "Failed to open output file '%s', aborting.", name);
                exit(EXIT_FAILURE);
            }
        }
        TSL_BUG_IF_FAILED(ais_decode_new(&ch[c].ais, center_freq, on_position_report, on_base_station_report,
                                         on_static_voyage_data));
        ais_decode_set_user(ch[c].ais, &ch[c]);
    }
    DEC_MSG(SEV_INFO, "PROTOCOL", "Using the AIS Message Format.");

    struct mfm_resampler *rs = NULL;
    struct mfm_ais *ais = NULL;
    struct mfm_resampler_config rc = { .abi_version = MFM_ABI_VERSION, .device = device, .nr_channels = nr_chan,
        .interpolate = interpolate, .decimate = decimate, .max_in_samples = block, .invert = invert,
        .dc_block = dc_blocker, .dc_pole = dc_block_pole };
    if (mfm_resampler_create(&rs, &rc, coeffs, nr_coeffs)) {
        DEC_MSG(SEV_FATAL, "NO-RESAMPLER", "Cannot create the GPU resampler: %s", mfm_last_error());
        exit(EXIT_FAILURE);
    }
    const uint32_t max_pcm = (uint32_t)mfm_resampler_max_out(rs);
    struct mfm_ais_config ac = { .abi_version = MFM_ABI_VERSION, .device = device, .nr_channels = nr_chan,
        .max_in_samples = max_pcm, .max_events = 0, .flags = 0 };
    if (mfm_ais_create(&ais, &ac)) {
        DEC_MSG(SEV_FATAL, "NO-AIS-STAGE", "Cannot create the GPU AIS stage: %s", mfm_last_error());
        exit(EXIT_FAILURE);
    }
    const size_t max_events = (size_t)nr_chan * (max_pcm / 160 + 16);
    struct mfm_ais_event *events = calloc(max_events, sizeof(*events));
    int16_t *pcm = calloc((size_t)nr_chan * block, sizeof(int16_t));
    TSL_BUG_ON(NULL == events || NULL == pcm);

    size_t sample_count = 0;
    for (;;) {
        size_t n = block;
        for (unsigned c = 0; c < nr_chan; c++) {
            ssize_t got = read_full(ch[c].fd, pcm + (size_t)c * block, (size_t)block * sizeof(int16_t));
            if (got < 0) {
                DEC_MSG(SEV_FATAL, "READ-FIFO-FAIL", "Failed to read from input fifo: %s (%d)", strerror(errno), errno);
                got = 0;
            }
            if ((size_t)got / sizeof(int16_t) < n) {
                n = (size_t)got / sizeof(int16_t);
            }
        }
        if (0 == n) {
            break;
        }
        int16_t *d_out = NULL;
        size_t out_stride = 0, nr_out = 0, nr_events = 0;
        if (sign_bits) {
            struct mfm_bits_view view;
            TSL_BUG_ON(MFM_OK != mfm_resampler_process_bits_host_to_device(rs, pcm, block, n, NULL, MFM_BITS_POS, &view));
            TSL_BUG_ON(MFM_OK != mfm_ais_process_bits_device(ais, &view, NULL));
        } else {
            TSL_BUG_ON(MFM_OK != mfm_resampler_process_host_to_device(rs, pcm, block, n, NULL, &d_out, &out_stride, &nr_out));
            TSL_BUG_ON(MFM_OK != mfm_ais_process_device(ais, d_out, out_stride, nr_out, NULL));
        }
        TSL_BUG_ON(MFM_OK != mfm_ais_fetch_events(ais, events, max_events, &nr_events));
        /* events come grouped by channel, in stream order inside a channel */
        size_t first = 0;
        while (first < nr_events) {
            size_t last = first;
            while (last < nr_events && events[last].channel == events[first].channel) {
                last++;
            }
            TSL_BUG_IF_FAILED(ais_decode_on_events(ch[events[first].channel].ais, &events[first], last - first));
            first = last;
        }
        sample_count += n;
        if (n < block) {
            break;
        }
    }
    DEC_MSG(SEV_INFO, "TERMINATING", "Terminating processing loop, processed %zu samples per channel", sample_count);

    mfm_ais_destroy(&ais);
    mfm_resampler_destroy(&rs);
    for (unsigned c = 0; c < nr_chan; c++) {
        DEC_MSG(SEV_INFO, "CRC-REJECTS", "Channel %u: %zu packets failed the FCS, %zu too short for their type", c,
                ais_decode_crc_rejects(ch[c].ais), ais_decode_short_packets(ch[c].ais));
        ais_decode_delete(&ch[c].ais);
        close(ch[c].fd);
        if (ch[c].out != stdout) {
            fclose(ch[c].out);
        } else {
            fflush(stdout);
        }
    }
    free(events);
    free(pcm);
    free(ch);
    free(coeffs);
    free(coeffs_f);
    config_delete(&cfg);
    return EXIT_SUCCESS;
}
